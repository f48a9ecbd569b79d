"""256 fragments per object (the reference's "-f256" models), host side: the oracles reproduce
the f256_* fixtures recorded from the imported reference (tests/golden/make_golden_f256.py,
make_graph_golden_f256.py), both readings of the network build the reference's graph at
num_frags = 256, and num_frags beyond 256 is refused. CPU only."""
import glob
import os

import numpy as np
import pytest

from oracle import corresp_ref, fragment_ref
from test_graph_trace import _ckpt, _diff, _load

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KEYS = ['px_id', 'frag_id', 'coord_2d', 'coord_3d', 'conf', 'conf_obj', 'conf_frag']
CASES = sorted(glob.glob(os.path.join(GOLDEN, 'f256_corresp_*.npz')))
GRAPH = os.path.join(GOLDEN, 'f256_graph_c2_xception65_640x480_o21.json')


def test_f256_fixtures_present():
  names = [os.path.basename(p) for p in CASES]
  assert len(names) == 8, names
  Fs = {np.load(p)['frag_confs'].shape[3] for p in CASES}
  assert Fs == {128, 200, 256}
  assert os.path.exists(os.path.join(GOLDEN, 'f256_fragment_ellipsoid_s2.npz'))
  assert os.path.exists(GRAPH)


@pytest.mark.parametrize('path', CASES, ids=[os.path.basename(p) for p in CASES])
def test_corresp_oracle_matches_f256_golden(path):
  z = np.load(path)
  num_objs = z['frag_centers'].shape[0]
  out = corresp_ref.establish_many_to_many(
      z['obj_confs'], z['frag_confs'], z['frag_coords'],
      gt_obj_ids=list(z['gt_obj_ids']), obj_ids=range(1, num_objs + 1),
      frag_centers={o + 1: z['frag_centers'][o] for o in range(num_objs)},
      frag_sizes={o + 1: z['frag_sizes'][o] for o in range(num_objs)},
      output_scale=float(z['output_scale']),
      min_obj_conf=float(z['min_obj_conf']),
      min_frag_rel_conf=float(z['min_frag_rel_conf']),
      only_annotated_objs=bool(z['only_annotated']))
  assert sorted(out.keys()) == sorted(int(o) for o in z['out_obj_ids'])
  for oid in out:
    for k in KEYS:
      exp = z['out_%d_%s' % (oid, k)]
      assert out[oid][k].dtype == exp.dtype, (oid, k)
      assert np.array_equal(out[oid][k], exp), (oid, k)


def test_f256_tie_case_drops_ties_across_mask_words():
  """Pixels (1,2) and (2,5) of object 1: conf == max * tau_b on fragments either side of the
  64-fragment word boundaries; only the strictly greater ones are kept, in ascending order."""
  z = np.load(os.path.join(GOLDEN, 'f256_corresp_o3_tie_s4.npz'))
  px2d = z['out_1_coord_2d']
  fr = z['out_1_frag_id']
  for (y, x), kept in (((1, 2), [64, 100, 127, 192, 255]),
                       ((2, 5), [0, 63, 100, 128, 191])):
    sel = (px2d[:, 0] == 4.0 * (x + 0.5)) & (px2d[:, 1] == 4.0 * (y + 0.5))
    assert list(fr[sel]) == kept


def test_fragment_oracle_matches_f256_golden():
  z = np.load(os.path.join(GOLDEN, 'f256_fragment_ellipsoid_s2.npz'))
  assert int(z['num_frags']) == 256
  centers, ids = fragment_ref.fragmentation_fps(z['vertices'], 256)
  assert np.array_equal(centers, z['frag_centers'])
  assert np.array_equal(ids, z['vertex_frag_ids'])


def test_oracle_net_builds_the_f256_reference_graph():
  from oracle import net_ref
  g = _load(GRAPH)
  cfg = g['config']
  assert cfg['num_frags'] == 256
  img = np.zeros((1, cfg['height'], cfg['width'], 3), np.float32)
  net_ref.DEVICE = 'meta'
  try:
    with net_ref.trace() as tr:
      net_ref.predict(img, _ckpt(cfg), num_objs=cfg['num_objs'], num_frags=cfg['num_frags'],
                      model_variant=cfg['model_variant'], multi_grid=cfg['multi_grid'],
                      atrous_rates=tuple(cfg['atrous_rates']),
                      encoder_output_stride=cfg['encoder_output_stride'],
                      decoder_output_stride=tuple(cfg['decoder_output_stride']))
  finally:
    net_ref.DEVICE = None
  assert tr.layers == g['layers'], _diff(g['layers'], tr.layers)[:5]
  assert tr.outputs == g['outputs']


def test_hip_plan_builds_the_f256_reference_graph():
  from epos_amd import net
  g = _load(GRAPH)
  cfg = g['config']
  plan = net.EposNet(_ckpt(cfg), 1, cfg['height'], cfg['width'], cfg['num_objs'],
                     cfg['num_frags'], model_variant=cfg['model_variant'],
                     multi_grid=cfg['multi_grid'], atrous_rates=tuple(cfg['atrous_rates']),
                     dry_run=True)
  d = _diff(g['layers'], plan.trace_layers)
  assert not d, d[:5]
  assert len(plan.trace_layers) == len(g['layers'])
  assert plan.trace_outputs == g['outputs']
  heads = {l['scope']: l['cout'] for l in g['layers'] if l['scope'].startswith('logits/')}
  assert heads == {'logits/pred_frag_conf': 21 * 256, 'logits/pred_frag_loc': 21 * 256 * 3,
                   'logits/pred_obj_conf': 22}
  launched = '+'.join(n for n, _ in plan.ops)
  for l in g['layers']:
    assert l['scope'] in launched, l['scope']
  # the sparse-head byte model leaves out exactly the dense fragment heads (4 B x 4F x O)
  drop = plan.algorithmic_bytes(True) - plan.algorithmic_bytes(False)
  assert drop == 4 * 120 * 160 * 21 * 256 * 4


@pytest.mark.parametrize('F', [0, 257, 512])
def test_num_frags_outside_1_256_is_refused(F):
  from epos_amd import net, weights
  ckpt = weights.random_init(num_objs=1, num_frags=max(F, 1), seed=0)
  with pytest.raises(ValueError, match=r'\[1, 256\]'):
    net.EposNet(ckpt, 1, 64, 64, 1, F, dry_run=True)
