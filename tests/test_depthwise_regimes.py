"""The shape table of tests/test_gpu_depthwise.py reaches every launch regime of
epos_depthwise3x3_f32 (CPU only: the regimes come from the host-side mirror in
tests/helpers/dw_regimes.py)."""
from helpers import dw_regimes as dr


def _regimes(shapes, **env):
  return {s.name: dr.shape_regime(s, **env) for s in shapes}


def test_mirror_matches_the_regimes_the_issue_table_names():
  """Spot values of the mirror, worked out by hand from layers.hip."""
  r = dr.regime(2, 61, 83, 728, 1, ldx=736, ldy=736)
  assert (r.kernel, r.rows, r.mode, r.unit, r.widths) == ('s1', 2, 0, 8, (16, 22, 24))
  r = dr.regime(2, 61, 83, 728, 1)
  assert (r.rows, r.mode, r.unit) == (2, 0, 1)
  r = dr.regime(1, 9, 11, 728, 2, ldx=736, ldy=736)
  assert (r.rows, r.mode, r.unit) == (1, 0, 8)
  r = dr.regime(2, 34, 45, 1536, 12)
  assert r.rows == 2 and 34 % 24 == 10 and r.nrows == 24
  r = dr.regime(1, 33, 45, 2048, 24)
  assert r.rows == 2 and r.nres == 24
  r = dr.regime(2, 10, 7, 728, 12, ldx=736, ldy=736)
  assert r.nres == 7 and r.nrows == 10
  # 4-float offset of the bases: not line-aligned although ld % 32 == 0
  assert dr.regime(1, 47, 61, 256, 1, ldx=256, ldy=256).unit == 8
  assert dr.regime(1, 47, 61, 256, 1, ldx=256, ldy=256, x_off=16, y_off=16).unit == 1
  assert dr.regime(2, 33, 47, 256, 1, stride=2).kernel == 'generic'
  # the switches
  assert dr.regime(1, 5, 6, 32, 8, rows_env=22).rows == 2
  assert dr.regime(2, 61, 83, 728, 1, rows_env=1).rows == 1
  assert dr.regime(3, 41, 57, 264, 5, mode_env=0).mode == 0
  assert dr.regime(2, 61, 83, 728, 1, mode_env=1).mode == 1
  assert dr.regime(1, 5, 6, 28, 8, mode_env=0).mode == 1      # c4n < 8: always bands


def test_depthwise_shape_table_covers_every_regime():
  regs = _regimes(dr.SHAPES)
  s1 = {n: r for n, r in regs.items() if r.kernel == 's1'}
  shape = {s.name: s for s in dr.SHAPES}
  combos = {(r.rows, r.mode, r.unit) for r in s1.values()}
  want = {(rows, 0, unit) for rows in (1, 2) for unit in (1, 8)} | \
      {(rows, 1, None) for rows in (1, 2)}
  assert want <= combos, sorted(want - combos, key=str)
  assert any(len(r.widths) == 3 for r in s1.values()), 'three distinct slice widths'
  assert any(r.nres < shape[n].rate for n, r in s1.items()), 'rate >= Wo'
  assert any(r.rows == 2 and shape[n].hi % (2 * shape[n].rate) != 0
             for n, r in s1.items()), 'ROWS = 2 with Ho % (2 rate) != 0'
  assert any(r.mode == 1 and r.rows == 2 and r.band_crosses_image and shape[n].b >= 2
             for n, r in s1.items()), 'ROWS = 2 row band across an image boundary'
  assert any(r.mode == 1 and r.rows == 1 and r.band_crosses_image
             for r in s1.values()), 'ROWS = 1 row band across an image boundary'
  assert any(r.dead_lanes for r in s1.values()), 'a last wave with dead lanes'
  gen = [shape[n] for n, r in regs.items() if r.kernel == 'generic']
  assert any(s.stride == 2 and s.c >= 256 for s in gen), 'stride 2 with C >= 256'
  assert any(s.stride == 2 and s.ldx != s.c for s in gen), 'stride 2 with ldx != C'
  assert any(s.off and r.unit == 1 and s.ldx % 32 == 0 and s.ldy % 32 == 0
             for s, r in ((shape[n], r) for n, r in s1.items())), 'unaligned bases'
  # the stray-write check needs padding columns in Y
  assert all(s.ldy > s.c or s.off for s in dr.SHAPES)


def test_every_switch_changes_the_regime_of_some_switch_shape():
  """Each EPOS_DW_* child run puts at least one problem into a regime its default run does
  not take (EPOS_DW_THREADS changes the workgroup size of every launch); EPOS_DW_ROWS=22
  reaches the two-row kernel with rate >= Ho."""
  base = _regimes(dr.SWITCH_SHAPES)
  shape = {s.name: s for s in dr.SWITCH_SHAPES}
  for env in dr.SWITCHES:
    if 'EPOS_DW_THREADS' in env:
      continue
    got = _regimes(dr.SWITCH_SHAPES, **dr.switch_env(env))
    changed = [n for n in base if (got[n].rows, got[n].mode) != (base[n].rows, base[n].mode)]
    assert changed, env
  got = _regimes(dr.SWITCH_SHAPES, rows_env=22)
  assert any(r.rows == 2 and shape[n].rate >= shape[n].hi for n, r in got.items())
  assert any(r.rows == 2 for r in base.values()) and any(r.rows == 1 for r in base.values())
