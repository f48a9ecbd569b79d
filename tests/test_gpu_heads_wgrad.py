"""epos_heads_wgrad_f32 and epos_momentum_step_f32 on the device (csrc/heads_wgrad.hip) and the
Python layer over them (epos_amd/heads_train.py). The reference for the logit gradients d is
the device's own epos_loss_grads output on the same inputs (pinned by test_gpu_loss_grad.py),
fed to tests/helpers/heads_wgrad_ref.py: the comparison is about the fp64 summation only, to
heads_wgrad_ref.bound. Outputs are pre-filled with a sentinel: every element must be written,
zeros as +0.0 bytes, and a skipped output untouched."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import heads_wgrad_ref as ref, loss_cases, loss_grad_ref      # noqa: E402
from tests.helpers import loss_device                                            # noqa: E402
from tests.helpers.loss_device import (IGNORE, KEYS, MEAN, NET_B, NET_F, NET_O,  # noqa: E402,F401
                                       POOLED, SENTINEL, UPSTREAM, WEIGHTS, _lib, _off, _out, _p,
                                       _stream, net_logits, ref_counts, small_net, tensors)

pytestmark = pytest.mark.gpu

HEADS = ref.HEADS
OUTS = [(h, j) for h in HEADS for j in (0, 1)]          # dW_obj, db_obj, dW_frag, ...


def features(n_pix, K, seed, lda=None):
  """(A f32 [n_pix, K], its padded copy [n_pix, lda] whose padding is NaN: never read)."""
  rng = np.random.RandomState(seed)
  A = (1.5 * rng.randn(n_pix, K)).astype(np.float32)
  A[rng.rand(n_pix, K) < 0.3] = 0.0                      # a ReLU output
  lda = K if lda is None else lda
  padded = np.full((n_pix, lda), np.nan, np.float32)
  padded[:, :K] = A
  return A, padded


class Device(object):
  """A host case on the device, with the logit gradients epos_loss_grads writes for it."""

  def __init__(self, c, A_padded, K, scale, upstream=None, ignore=IGNORE, in_off=(0, 0, 0, 0)):
    self.c, self.K, self.ignore = c, K, ignore
    self.B, self.P, O1 = c['obj_logits'].shape
    self.O, self.F = c['frag_logits'].shape[2:4]
    self.lda, self.ld_obj = A_padded.shape[1], O1
    self.A = _off(A_padded, in_off[0])
    self.obj = _off(c['obj_logits'], in_off[1])
    self.frag = _off(c['frag_logits'], in_off[2])
    self.loc = _off(c['frag_loc'], in_off[3])
    self.g_obj = _off(np.asarray(c['gt_obj'], np.int32), in_off[1], torch.int32)
    self.g_frag = _off(np.asarray(c['gt_frag'], np.int32), in_off[2], torch.int32)
    self.g_loc = _off(np.asarray(c['gt_loc'], np.float32), in_off[3])
    self.g_w = _off(np.asarray(c['gt_weight'], np.float32), in_off[0])
    self.sc = torch.from_numpy(np.ascontiguousarray(scale, np.float64)).cuda()
    self.up = None if upstream is None else torch.tensor(upstream, dtype=torch.float64,
                                                         device='cuda')
    self.widths = {'obj': O1, 'frag': self.O * self.F, 'loc': self.O * self.F * 3}
    self._ref = None

  def logit_grads(self):
    return loss_device.logit_grads(self)

  def reference(self):
    """(sums, abs_sums, n_terms) of heads_wgrad_ref.wgrads on the device's own d."""
    if self._ref is None:
      d = [t.cpu().numpy() for t in self.logit_grads()]
      B, P, O, F = self.B, self.P, self.O, self.F
      A = self.A.cpu().numpy().reshape(B * P, self.lda)[:, :self.K]
      cls, frag = ref.classes(self.c, self.ignore)
      self._ref = ref.wgrads(A, d[0].reshape(B * P, O + 1), d[1].reshape(B * P, O, F),
                             d[2].reshape(B * P, O, F, 3), cls, frag)
    return self._ref

  def run(self, want=(True,) * 6, out_off=(0,) * 6, B=None, P=None, null_inputs=False):
    """One call. Returns {(head, j): uint32 bits} of the outputs asked for; an output not asked
    for must still hold the sentinel."""
    lib = _lib()
    B = self.B if B is None else B
    P = self.P if P is None else P
    nbytes = lib.epos_heads_wgrad_workspace_bytes(B, P, self.O, self.F, self.K)
    assert 20 * B * P <= nbytes < max(1, 4 * B * P * (self.O + 1 + 4 * self.O * self.F))
    ws = torch.full((nbytes // 8 + 1,), -1, dtype=torch.int64, device='cuda')
    bufs = [_out((self.K if j == 0 else 1) * self.widths[h], off)
            for (h, j), off in zip(OUTS, out_off)]
    ptrs = [_p(b) if w else None for b, w in zip(bufs, want)]
    ins = [self.A, self.obj, self.frag, self.loc, self.g_obj, self.g_frag, self.g_loc, self.g_w,
           self.sc, ws]
    ip = [None if null_inputs else _p(t) for t in ins]
    rc = lib.epos_heads_wgrad_f32(ip[0], self.lda, self.K, ip[1], self.O + 1, ip[2], ip[3], ip[4],
                                  ip[5], ip[6], ip[7], B, P, self.O, self.F, self.ignore, ip[8],
                                  None if null_inputs else _p(self.up), ip[9], *ptrs, _stream())
    assert rc == 0, lib.epos_last_error()
    torch.cuda.synchronize()
    got = {}
    for key, b, w in zip(OUTS, bufs, want):
      raw = b.view(torch.int32).cpu().numpy().view(np.uint32)
      if not w:
        assert (raw == SENTINEL).all(), key               # not asked for: not touched
        continue
      assert not (raw == SENTINEL).any(), key             # every element is written
      got[key] = raw.reshape(self.K, -1) if key[1] == 0 else raw
    return got

  def check(self, got):
    """Every output of `got` against the reference, to bound; columns nobody adds to are +0.0
    bytes. Returns the worst error / bound."""
    sums, abs_sums, n_terms = self.reference()
    worst = 0.0
    for (h, j), bits in got.items():
      empty = n_terms[h] == 0
      assert not bits[..., empty].any(), (h, j)           # +0.0, not -0.0
      ok, w = ref.within(bits.view(np.float32), sums[h][j], abs_sums[h][j], n_terms[h])
      assert ok, (h, j, w)
      worst = max(worst, w)
    return worst


def make(B, P, O, F, K, seed, reduction=MEAN, upstream=None, lda=None, empty_images=(),
         in_off=(0, 0, 0, 0), edit=None):
  c = loss_cases.make_case(B, P, O, F, seed, empty_images=empty_images)
  A, padded = features(B * P, K, seed + 1, lda)
  if edit is not None:
    edit(c, padded)
  scale = loss_grad_ref.scales(ref_counts(c), WEIGHTS, reduction)
  return Device(c, padded, K, scale, upstream, in_off=in_off)


@pytest.mark.parametrize('O', [1, 3, 21])
@pytest.mark.parametrize('F', [1, 3, 4, 63, 64, 65, 256])
def test_sweep(F, O):
  # images this small are one range (range_pixels == P; test_pixel_ranges has the larger ones),
  # so P runs through the scan step and the batch sizes: one pixel, a short wave, one more than
  # a wave, more than a batch
  lib = _lib()
  sizes = [1, 63, 64, 65, 257]
  Ks = [1, 3, 64, 256] if O * F <= 192 else [8, 3]
  for i, P in enumerate(sizes):
    K = Ks[(i + O + F) % len(Ks)]
    assert lib.epos_heads_wgrad_range_pixels(P, O, F, K) == P
    lda = K + 3 * ((i + F) % 2)
    # both reductions, with and without upstream, in turn over the sizes
    reduction, upstream = ((MEAN, UPSTREAM), (POOLED, None), (MEAN, None), (POOLED, UPSTREAM))[
        (i + O) % 4]
    dev = make(3, P, O, F, K, seed=1000 * F + 10 * O + i, reduction=reduction,
               upstream=upstream, lda=lda, empty_images=(1,))
    worst = dev.check(dev.run())
    print('O %d F %d P %d K %d lda %d reduction %d: worst error / bound %.3f' % (
        O, F, P, K, lda, reduction, worst))


@pytest.mark.parametrize('P', [2047, 2048, 2049, 3073, 8200])
def test_pixel_ranges(P):
  # K = 3: ranges of at least 1024 pixels. 2047: one range; 2048: two of r = 1024; 2049: r and
  # r - 1; 3073: three, the last one r - 2; 8200: eight. Each range ends inside a scan step.
  lib = _lib()
  O, F, K = 3, 5, 3
  R = min(8, P // 1024)
  r = int(lib.epos_heads_wgrad_range_pixels(P, O, F, K))
  assert r == -(-P // R) and (R - 1) * r < P
  upstream, reduction = (UPSTREAM, MEAN) if P % 2 else (None, POOLED)
  dev = make(3, P, O, F, K, seed=P, reduction=reduction, upstream=upstream, lda=K + 3,
             empty_images=(1,))
  got = dev.run()
  print('P %d R %d r %d: worst error / bound %.3f' % (P, R, r, dev.check(got)))
  again = dev.run()
  for key in got:
    assert got[key].tobytes() == again[key].tobytes(), key
  for want in ((True, False, False, True, True, False), (False, True, False, False, False, True)):
    part = dev.run(want=want)                              # slabs of skipped outputs are not read
    for key, bits in part.items():
      assert bits.tobytes() == got[key].tobytes(), (want, key)


@pytest.mark.parametrize('K,lda', [(1, 1), (3, 6), (64, 64), (256, 259), (1024, 1024)])
def test_every_k(K, lda):
  dev = make(3, 130, 3, 8, K, seed=K, lda=lda, empty_images=(1,), upstream=UPSTREAM)
  dev.check(dev.run())


def test_objects_and_fragments():
  # object 1 without a pixel, object 2 with exactly one, object 3 with every one of its many
  # pixels on fragment 2 (the longest single run), object 4 as drawn; fragment 4 never assigned
  O, F, K, P = 4, 5, 19, 1500

  def edit(c, A):
    g = c['gt_obj']
    g[g == 1] = 0
    g[g == 2] = 4
    g[0, 700:1400] = 3
    g[0, 77] = 2
    fg = (g >= 1) & (g <= O)
    c['gt_frag'][:] = np.where(fg, np.where(c['gt_frag'] == 4, 0, np.abs(c['gt_frag'])), -1)
    c['gt_frag'][g == 3] = 2
    c['gt_weight'][:] = np.where(fg, np.maximum(c['gt_weight'], 0.25), 0.0)
  dev = make(2, P, O, F, K, seed=7, edit=edit)
  got = dev.run()
  dev.check(got)
  n = dev.reference()[2]
  nf, nl = n['frag'].reshape(O, F), n['loc'].reshape(O, F, 3)
  assert not nf[0].any() and (nf[1] == 1).all() and (nf[2] >= 700).all()
  assert nl[2, 2, 0] == nf[2, 0] and not nl[2, [0, 1, 3, 4]].any() and not nl[:, 4].any()
  assert nl[1].sum() == 3
  dWf = got[('frag', 0)].reshape(K, O, F)
  assert not dWf[:, 0].any() and got[('frag', 1)].reshape(O, F)[1].all()


VIEW_OFFS = [((1, 0, 0, 0), (0,) * 6), ((0, 2, 0, 0), (0,) * 6), ((0, 0, 3, 0), (0,) * 6),
             ((0, 0, 0, 1), (0,) * 6), ((0,) * 4, (1, 0, 2, 0, 3, 0)),
             ((0,) * 4, (0, 3, 0, 1, 0, 2)), ((3, 1, 2, 3), (2, 3, 1, 1, 3, 2))]


def test_views_and_alignment():
  B, P, O, F, K = 2, 150, 3, 7, 13
  base = make(B, P, O, F, K, seed=21, lda=K + 3, upstream=UPSTREAM)
  exp = base.run()
  base.check(exp)
  for in_off, out_off in VIEW_OFFS:
    dev = make(B, P, O, F, K, seed=21, lda=K + 3, upstream=UPSTREAM, in_off=in_off)
    got = dev.run(out_off=out_off)
    for key in exp:                                        # the same bytes at every offset
      assert got[key].tobytes() == exp[key].tobytes(), (in_off, out_off, key)


def test_null_outputs():
  # every combination of the six outputs: dW without db, db without dW, whole heads skipped
  dev = make(2, 90, 3, 6, 21, seed=22)
  exp = dev.run()
  dev.check(exp)
  for want in itertools.product([True, False], repeat=6):
    got = dev.run(want=want)
    assert set(got) == {k for k, w in zip(OUTS, want) if w}
    for key, bits in got.items():
      assert bits.tobytes() == exp[key].tobytes(), (want, key)


def test_empty_batch_writes_zeros():
  dev = make(2, 10, 3, 6, 5, seed=23)
  for kwargs in ({'P': 0}, {'B': 0}, {'P': 0, 'null_inputs': True}):
    got = dev.run(**kwargs)
    assert len(got) == 6 and not any(bits.any() for bits in got.values()), kwargs


def test_ignored_and_bad_pixels_contribute_nothing():
  O, F, K, P = 3, 6, 9, 120
  bad_pixels = []

  def edit(c, A):
    g, f, w = c['gt_obj'][0], c['gt_frag'][0], c['gt_weight'][0]
    g[20], g[21] = -1, O + 1                               # labels outside 0..O
    g[22:28] = 2
    f[22], f[23] = -1, F                                   # fragment outside 0..F-1
    w[24], w[25], w[26], w[27] = 0.0, -1.0, np.nan, np.inf
    f[24:28] = 1
    bad_pixels.extend(range(20, 28))
    ignored = list(np.nonzero(g == IGNORE)[0])
    assert ignored
    for p in bad_pixels + ignored:                         # must never be added
      A[p, :K] = np.nan
      c['obj_logits'][0, p] = np.nan
      c['frag_logits'][0, p] = np.inf
      c['frag_loc'][0, p] = np.nan
  dev = make(2, P, O, F, K, seed=24, lda=K + 3, edit=edit)
  cls = ref.classes(dev.c, IGNORE)[0]
  assert (cls[20:28] == -1).all()
  got = dev.run()
  dev.check(got)
  for bits in got.values():
    assert np.isfinite(bits.view(np.float32)).all()


@pytest.mark.parametrize('value', [np.nan, np.inf])
@pytest.mark.parametrize('where', ['feature', 'obj', 'frag', 'loc'])
def test_non_finite_value_marks_only_the_columns_it_touches(where, value):
  O, F, K, P = 3, 6, 9, 100
  c0 = loss_cases.make_case(1, P, O, F, 25)
  p = int(np.nonzero(c0['gt_obj'][0] == 2)[0][0])
  f = int(c0['gt_frag'][0, p])

  def edit(c, A):
    if where == 'feature':
      A[p, 4] = value
    elif where == 'obj':
      c['obj_logits'][0, p, 1] = value
    elif where == 'frag':
      c['frag_logits'][0, p, 1, 0] = value
    else:
      c['frag_loc'][0, p, 1, f, 2] = value
  dev = make(1, P, O, F, K, seed=25, edit=edit)
  got = dev.run()
  dev.check(got)                                           # non-finite where the reference is
  bad = {key: ~np.isfinite(bits.view(np.float32)) for key, bits in got.items()}
  cols_f = np.zeros((O, F), bool)
  cols_f[1] = True
  cols_l = np.zeros((O, F, 3), bool)
  cols_l[1, f] = True
  if where == 'feature':                                   # row 4 of the pixel's columns
    for h, cols in (('obj', np.ones(O + 1, bool)), ('frag', cols_f.reshape(-1)),
                    ('loc', cols_l.reshape(-1))):
      exp = np.zeros((K, cols.size), bool)
      exp[4] = cols
      assert (bad[(h, 0)] == exp).all(), h
      assert not bad[(h, 1)].any()
  else:
    assert bad[('obj', 0)].all() == (where == 'obj') and bad[('obj', 1)].all() == (where == 'obj')
    assert bad[('obj', 0)].any() == (where == 'obj')
    assert (bad[('frag', 1)] == (cols_f.reshape(-1) & (where == 'frag'))).all()
    assert (bad[('frag', 0)] == (cols_f.reshape(-1) & (where == 'frag'))[None, :]).all()
    if where == 'loc' and np.isinf(value):                 # the clamp makes an infinity finite
      assert not bad[('loc', 0)].any() and not bad[('loc', 1)].any()
    else:
      one = np.zeros((O, F, 3), bool)
      one[1, f, 2] = where == 'loc'
      assert (bad[('loc', 1)] == one.reshape(-1)).all()


def test_determinism_and_image_order():
  B, P, O, F, K = 3, 700, 3, 64, 40
  dev = make(B, P, O, F, K, seed=26, upstream=UPSTREAM)
  a, b = dev.run(), dev.run()
  for key in a:
    assert a[key].tobytes() == b[key].tobytes(), key
  dev.check(a)
  # the images permuted: another order of the same sums
  perm = [2, 0, 1]
  c2 = {k: np.ascontiguousarray(v[perm]) for k, v in dev.c.items()}
  A = dev.A.cpu().numpy().reshape(B, P, K)[perm].reshape(B * P, K)
  dev2 = Device(c2, A, K, dev.sc.cpu().numpy()[perm], UPSTREAM)
  got = dev2.run()
  sums, abs_sums, n_terms = dev.reference()
  for (h, j), bits in got.items():
    ok, w = ref.within(bits.view(np.float32), sums[h][j], abs_sums[h][j], n_terms[h])
    assert ok, (h, j, w)


def test_against_the_dense_route_on_the_device():
  B, P, O, F, K = 2, 1200, 3, 64, 64
  dev = make(B, P, O, F, K, seed=27, reduction=POOLED)
  got = dev.run()
  d = dev.logit_grads()
  A64 = dev.A.view(B * P, K).double()
  _, abs_sums, n_terms = dev.reference()
  for h, t in zip(HEADS, d):
    d64 = t.view(B * P, -1).double()
    dense = (A64.t() @ d64).cpu().numpy(), d64.sum(dim=0).cpu().numpy()
    for j in (0, 1):
      ok, w = ref.within(got[(h, j)].view(np.float32), dense[j], abs_sums[h][j], n_terms[h])
      assert ok, (h, j, w)


@pytest.mark.parametrize('O,F,K,fg', [(3, 8, 24, False), (3, 8, 24, True), (2, 65, 5, True)])
def test_one_pixel_gives_the_logit_gradients_themselves(O, F, K, fg):
  # B = P = 1: every sum has a single term, and with features that are powers of two,
  # A[k] = 2^(k % 5 - 2), that term is exact: dW[k, col] == A[k] * d[col] and db[col] == d[col]
  # for d = epos_loss_grads' output on the same inputs, for all six outputs (as fp32 values).
  # That holds only while both round an element with the same function. A background pixel, a
  # foreground pixel, and one at F > 64: four feature indices per slice, fragment 64.
  def edit(c, A):
    A[0, :K] = 2.0 ** (np.arange(K) % 5 - 2)
    if fg:
      c['gt_obj'][0, 0], c['gt_frag'][0, 0], c['gt_weight'][0, 0] = O, F - 1, 0.75
    else:
      c['gt_obj'][0, 0], c['gt_frag'][0, 0], c['gt_weight'][0, 0] = 0, -1, 0.0
  dev = make(1, 1, O, F, K, seed=70 + F, lda=K + 3, edit=edit)
  assert ref.classes(dev.c, IGNORE)[0].tolist() == [O if fg else 0]
  got = dev.run()
  A = dev.A.cpu().numpy().reshape(1, dev.lda)[0, :K]
  for h, t in zip(HEADS, dev.logit_grads()):
    d = t.cpu().numpy()
    assert np.isfinite(d).all() and d.any() == (fg or h == 'obj')
    dW, db = got[(h, 0)].view(np.float32), got[(h, 1)].view(np.float32)
    assert (dW == A[:, None] * d[None, :]).all() and (db == d).all(), h


# ---------------------------------------------------------------- momentum step ---
HYPER = [(0.01, 0.9, 4e-5, 1.0), (0.5, 0.0, 0.0, 1.0), (0.003, 0.9, 0.0, 2.0),
         (0.1, 0.5, 0.01, 2.0)]


@pytest.mark.parametrize('n', [0, 1, 3, 4, 5, 1023, 1024, 1025, 2 ** 20 + 3])
def test_momentum_step_bytes(n):
  lib = _lib()
  rng = np.random.RandomState(n % 1000)
  w, a, g = (rng.randn(n).astype(np.float32) for _ in range(3))
  offsets = [(o, o, o) for o in range(4)] + [(1, 2, 3), (0, 0, 2)]
  for i, off in enumerate(offsets):
    lr, mom, wd, gm = HYPER[i % len(HYPER)]
    dw, da, dg = (_off(x, o) for x, o in zip((w, a, g), off))
    guard = [t.clone() for t in (dw, da)]
    rc = lib.epos_momentum_step_f32(_p(dw), _p(da), _p(dg), n, lr, mom, wd, gm, _stream())
    assert rc == 0, lib.epos_last_error()
    torch.cuda.synchronize()
    w2, a2 = ref.momentum_step(w, a, g, lr, mom, wd, gm)
    assert dw.cpu().numpy().tobytes() == w2.tobytes(), (n, off)
    assert da.cpu().numpy().tobytes() == a2.tobytes(), (n, off)
    assert torch.equal(dg.cpu(), torch.from_numpy(g))
    if n:
      assert not torch.equal(dw, guard[0])


# ---------------------------------------------------------------- through Python ---
def test_heads_weight_grads_entry():
  from epos_amd import heads_train, loss
  B, h, w, O, F, K = 2, 9, 11, 3, 8, 24
  dev = make(B, h * w, O, F, K, seed=31, lda=K + 8, upstream=UPSTREAM)
  exp = dev.run()
  logits, gt = tensors(dev.c, h, w)
  feats = dev.A.view(B, h, w, K + 8)[..., :K]              # a view of a wider buffer
  up = torch.tensor(UPSTREAM, dtype=torch.float64, device='cuda')
  res = heads_train.heads_weight_grads(feats, logits, gt, dev.sc, upstream=up)
  assert set(res) == set(KEYS)
  for name, head in zip(KEYS, HEADS):
    dW, db = res[name]
    assert dW.dtype == torch.float32 and tuple(dW.shape) == (K, dev.widths[head])
    assert tuple(db.shape) == (dev.widths[head],)
    assert dW.cpu().numpy().tobytes() == exp[(head, 0)].tobytes()
    assert db.cpu().numpy().tobytes() == exp[(head, 1)].tobytes()
  # need, out and workspace
  ws = torch.empty((_lib().epos_heads_wgrad_workspace_bytes(B, h * w, O, F, K) // 8 + 1,),
                   dtype=torch.int64, device='cuda')
  mine = torch.full((K, O * F), -7.0, device='cuda')
  res2 = heads_train.heads_weight_grads(feats, logits, gt, dev.sc, upstream=up,
                                        need=(False, True, True),
                                        out={'pred_frag_conf': (mine, None)}, workspace=ws)
  assert res2['pred_obj_conf'] is None and res2['pred_frag_conf'][0] is mine
  assert res2['pred_frag_conf'][1] is None
  assert torch.equal(mine, res['pred_frag_conf'][0])
  assert torch.equal(res2['pred_frag_loc'][1], res['pred_frag_loc'][1])
  with pytest.raises(TypeError, match='bf16 decoder_out is not supported'):
    heads_train.heads_weight_grads(feats.bfloat16(), logits, gt, dev.sc)
  with pytest.raises(ValueError, match='features hold'):
    heads_train.heads_weight_grads(feats[:1], logits, gt, dev.sc)
  with pytest.raises(ValueError, match='workspace must be'):
    heads_train.heads_weight_grads(feats, logits, gt, dev.sc, workspace=ws[:3])
  assert loss.REDUCTIONS == {'mean': 0, 'pooled': 1}


def test_net_grads_of_the_logits_layers_on_a_real_net(small_net):
  from epos_amd import heads_train, loss, trainer
  net, ckpt, _, c, gt = small_net
  B, h, w, O, F = NET_B, net.out_h, net.out_w, NET_O, NET_F
  K = int(net.decoder_out.shape[-1])
  values, bad, grads = trainer.net_grads(net, gt, {}, weights=WEIGHTS, reduction='pooled')
  assert values.shape == (4,) and values.dtype == torch.float64 and bad.tolist() == [0] * B
  widths = dict(zip(KEYS, (O + 1, O * F, O * F * 3)))
  assert set(grads) == {n for k in KEYS for n in heads_train.variable_names(k)}
  for k in KEYS:
    wname, bname = heads_train.variable_names(k)
    assert tuple(grads[wname].shape) == (1, 1, K, widths[k]) == ckpt[wname].shape
    assert tuple(grads[bname].shape) == (widths[k],) == ckpt[bname].shape
  # the same as the three calls by hand
  logits = net_logits(net)
  sums, counts, _ = loss.loss_terms(logits, gt)
  values2, scales = loss.loss_values(sums, counts, WEIGHTS, 'pooled')
  assert torch.equal(values, values2)
  hand = heads_train.heads_weight_grads(net.decoder_out, logits, gt, scales)
  for k in KEYS:
    wname, bname = heads_train.variable_names(k)
    assert torch.equal(hand[k][0], grads[wname].view(K, -1))
    assert torch.equal(hand[k][1], grads[bname])
  # torch's autograd of differentiable_losses through an fp64 linear layer whose values are
  # pinned to the net's own logits: W.grad = A64^T d64 with d = epos_loss_grads' output
  A64 = net.decoder_out.reshape(B * h * w, K).double()
  Ws = {k: torch.from_numpy(ckpt[heads_train.variable_names(k)[0]]).cuda().double().view(
      K, -1).requires_grad_() for k in KEYS}
  bs = {k: torch.from_numpy(ckpt[heads_train.variable_names(k)[1]]).cuda().double()
        .requires_grad_() for k in KEYS}
  leaves = {}
  for k in KEYS:
    lin = (A64 @ Ws[k] + bs[k]).view(logits[k].shape)
    with torch.no_grad():                                  # the net's GEMM against fp64
      assert float((lin - logits[k]).abs().max()) < 1e-2 * max(1.0, float(lin.abs().max()))
    leaves[k] = (lin + (logits[k].double() - lin).detach()).float()
  v, _ = loss.differentiable_losses(leaves, gt, WEIGHTS, 'pooled')
  assert torch.equal(v.detach(), values)
  v[3].backward()
  d = loss.loss_grads(logits, gt, scales)
  cls, frag = ref.classes(c, IGNORE)
  _, abs_sums, n_terms = ref.wgrads(
      A64.cpu().numpy(), *[t.cpu().numpy().reshape(c[n].shape) for t, n in zip(
          d, ('obj_logits', 'frag_logits', 'frag_loc'))], cls, frag)
  for k, head in zip(KEYS, HEADS):
    wname, bname = heads_train.variable_names(k)
    for got, exp, j in ((grads[wname].view(K, -1), Ws[k].grad, 0), (grads[bname], bs[k].grad, 1)):
      assert exp.abs().max() > 0
      ok, worst = ref.within(got.cpu().numpy(), exp.cpu().numpy(), abs_sums[head][j],
                             n_terms[head])
      assert ok, (k, j, worst)


def test_descent_and_checkpoint(small_net, tmp_path):
  # the total is convex in (W, b) with a gradient that is L-Lipschitz, L <= lip * lambda_max of
  # the Gram matrix of [A 1]: lip bounds a pixel's Hessian in its logits (a cross-entropy row's
  # is <= 1/2, the Huber term's <= 1; test_gpu_loss_grad.test_descent_on_the_logits). A step of
  # 1/(2L) on the weights and, with the biases' multiplier 2, 1/L on the biases stays below 2/L,
  # so it must decrease the total strictly while the gradient is not zero.
  from epos_amd import heads_train, loss, tf_checkpoint, trainer
  net, ckpt, _, c, gt = small_net
  B, h, w, O, F = NET_B, net.out_h, net.out_w, NET_O, NET_F
  P = h * w
  A = net.decoder_out.reshape(B * P, -1).clone()
  K = A.shape[1]
  counts = ref_counts(c)
  n_min = int(counts[:, 1:, 0].sum(axis=1).min())
  w_max = float(c['gt_weight'].max())
  assert n_min > 0
  weights = (1.0, 1.0, 100.0)
  lip = max(weights[0] / (2 * P), weights[1] / (2 * n_min),
            weights[2] * w_max / (3 * n_min)) / B
  A1 = torch.cat([A.double(), torch.ones((B * P, 1), dtype=torch.float64, device='cuda')], dim=1)
  lam = float(np.linalg.eigvalsh((A1.t() @ A1).cpu().numpy())[-1])
  opt = trainer.Optimizer(ckpt, lr=0.5 / (lip * lam), momentum=0.0, weight_decay=0.0)
  shapes = {'pred_obj_conf': (B, h, w, O + 1), 'pred_frag_conf': (B, h, w, O, F),
            'pred_frag_loc': (B, h, w, O, F, 3)}
  totals = []
  for step in range(4):
    logits = {}
    for k in KEYS:
      wname, bname = heads_train.variable_names(k)
      logits[k] = (A @ opt.params[wname].view(K, -1) + opt.params[bname]).view(shapes[k])
    sums, counts_d, bad = loss.loss_terms(logits, gt)
    values, scales = loss.loss_values(sums, counts_d, weights, 'mean')
    totals.append(float(values[3]))
    if step == 3:
      break
    raw = heads_train.heads_weight_grads(A, logits, gt, scales)
    grads = {}
    for k in KEYS:
      wname, bname = heads_train.variable_names(k)
      grads[wname], grads[bname] = raw[k][0].view(1, 1, K, -1), raw[k][1]
    opt.step(grads)
  assert not bad.any()
  print('totals', totals)
  assert totals[1] < totals[0] and totals[2] < totals[1] and totals[3] < totals[2], totals
  # the state round-trips through a checkpoint under the names infer.py restores
  state = opt.state()
  for k in KEYS:
    for name in heads_train.variable_names(k):
      assert state[name].shape == ckpt[name].shape and state[name].dtype == np.float32
      assert not np.array_equal(state[name], ckpt[name])
      assert state[name + '/Momentum'].shape == ckpt[name].shape
  prefix = str(tmp_path / 'model.ckpt-3')
  tf_checkpoint.write_checkpoint(prefix, state)
  back = tf_checkpoint.load_checkpoint(prefix)
  assert set(back) == set(state)
  for name in state:
    assert back[name].tobytes() == state[name].tobytes() and back[name].shape == state[name].shape
  kept = tf_checkpoint.to_epos_checkpoint(back)
  assert set(kept) == {n for k in KEYS for n in heads_train.variable_names(k)}
  merged = dict(ckpt, **kept)                              # what a new net would be built from
  assert set(merged) == set(ckpt)


def test_optimizer_multipliers():
  from epos_amd import heads_train, trainer
  rng = np.random.RandomState(3)
  K, O, F = 5, 2, 3
  variables, grads = {}, {}
  for k, n in zip(KEYS, (O + 1, O * F, O * F * 3)):
    wname, bname = heads_train.variable_names(k)
    variables[wname] = rng.randn(1, 1, K, n).astype(np.float32)
    variables[bname] = rng.randn(n).astype(np.float32)
  opt = trainer.Optimizer(variables, lr=0.01, momentum=0.9, weight_decay=4e-5,
                          last_layer_gradient_multiplier=10.0)
  exp = {n: (v.copy(), np.zeros_like(v)) for n, v in variables.items()}
  for step in range(2):
    for n in variables:
      grads[n] = torch.from_numpy(rng.randn(*variables[n].shape).astype(np.float32)).cuda()
    opt.step(grads)
    for n in variables:
      bias = n.endswith('/biases')
      exp[n] = ref.momentum_step(exp[n][0], exp[n][1], grads[n].cpu().numpy(), 0.01, 0.9,
                                 0.0 if bias else 4e-5, 20.0 if bias else 10.0)
  state = opt.state()
  for n in variables:
    assert state[n].tobytes() == exp[n][0].tobytes(), n
    assert state[n + '/Momentum'].tobytes() == exp[n][1].tobytes(), n
  assert set(opt.state(with_slots=False)) == set(variables)


def test_capture_in_a_graph():
  from epos_amd import heads_train
  B, h, w, O, F, K = 2, 6, 7, 3, 8, 20
  dev = make(B, h * w, O, F, K, seed=35)
  logits, gt = tensors(dev.c, h, w)
  feats = dev.A.view(B, h, w, K)
  eager = heads_train.heads_weight_grads(feats, logits, gt, dev.sc)
  param0 = torch.from_numpy(np.random.RandomState(1).randn(K, O * F).astype(np.float32)).cuda()
  p_eager, a_eager = param0.clone(), torch.zeros_like(param0)
  heads_train.momentum_step(p_eager, a_eager, eager['pred_frag_conf'][0], 0.1, 0.9, 1e-4, 1.0)
  torch.cuda.synchronize()
  side = torch.cuda.Stream()
  out = {k: tuple(torch.full_like(t, -7.0) for t in eager[k]) for k in KEYS}
  ws = torch.empty((_lib().epos_heads_wgrad_workspace_bytes(B, h * w, O, F, K) // 8 + 1,),
                   dtype=torch.int64, device='cuda')
  param, accum = param0.clone(), torch.zeros_like(param0)
  with torch.cuda.stream(side):                            # warm-up outside the capture
    heads_train.heads_weight_grads(feats, logits, gt, dev.sc, out=out, workspace=ws)
  torch.cuda.synchronize()
  for pair in out.values():
    for t in pair:
      t.fill_(-7.0)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    heads_train.heads_weight_grads(feats, logits, gt, dev.sc, out=out, workspace=ws)
    heads_train.momentum_step(param, accum, out['pred_frag_conf'][0], 0.1, 0.9, 1e-4, 1.0)
  graph.replay()
  torch.cuda.synchronize()
  for k in KEYS:
    for a, b in zip(out[k], eager[k]):
      assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), k
  assert torch.equal(param, p_eager) and torch.equal(accum, a_eager)
