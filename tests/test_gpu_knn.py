"""gt_knn_frags > 1 on the device (include/epos_hip.h, "k nearest fragments"): the six _knn
entries through the C ABI against tests/helpers/knn_ref.py at the smallest shapes where the
kernels can go wrong, and the six old entries against their siblings at k = 1, byte for byte.
Outputs are pre-filled with a sentinel: every element must be written."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import (heads_dgrad_ref, heads_wgrad_ref, knn_ref, loss_cases,    # noqa: E402
                           loss_grad_ref, loss_ref)
from tests.helpers.loss_device import (IGNORE, MEAN, POOLED, SENTINEL, UPSTREAM,     # noqa: E402
                                       WEIGHTS, _lib, _off, _out, _p, _stream)

pytestmark = pytest.mark.gpu

INVALID = -1
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'knn_frags.npz')


def _bits(t):
  return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------ ground truth ---
def run_gt(depth, local_pos, masks, obj_ids, centers, sizes, knn, old=False):
  """epos_gt_fields_knn (old: epos_gt_fields, knn == 1) -> dict of numpy arrays."""
  lib = _lib()
  n, h, w = depth.shape
  O, F = sizes.shape
  d = torch.from_numpy(np.ascontiguousarray(depth, np.float32)).cuda()
  lp = torch.from_numpy(np.ascontiguousarray(local_pos, np.float32)).cuda()
  m = None if masks is None else torch.from_numpy(np.ascontiguousarray(masks, np.uint8)).cuda()
  ids = torch.tensor(list(obj_ids), dtype=torch.int32, device='cuda')
  c = torch.from_numpy(np.ascontiguousarray(centers, np.float64)).cuda()
  s = torch.from_numpy(np.ascontiguousarray(sizes, np.float64)).cuda()
  out = {'obj_label': torch.full((h, w), -9, dtype=torch.int32, device='cuda'),
         'instance': torch.full((h, w), -9, dtype=torch.int32, device='cuda'),
         'frag_label': torch.full((h, w, knn), -9, dtype=torch.int32, device='cuda'),
         'frag_loc': _out(h * w * knn * 3, 0).view(h, w, knn, 3),
         'frag_weight': _out(h * w * knn, 0).view(h, w, knn)}
  outs = [_p(out[k]) for k in ('obj_label', 'instance', 'frag_label', 'frag_loc', 'frag_weight')]
  if old:
    assert knn == 1
    rc = lib.epos_gt_fields(_p(d), _p(lp), _p(m), _p(ids), n, h, w, _p(c), _p(s), O, F, *outs,
                            _stream())
  else:
    rc = lib.epos_gt_fields_knn(_p(d), _p(lp), _p(m), _p(ids), n, h, w, _p(c), _p(s), O, F, knn,
                                *outs, _stream())
  assert rc == 0, lib.epos_last_error()
  torch.cuda.synchronize()
  return {k: v.cpu().numpy() for k, v in out.items()}


def same_fields(got, exp):
  for k in exp:
    assert got[k].shape == exp[k].shape and got[k].dtype == exp[k].dtype, k
    assert got[k].tobytes() == exp[k].tobytes(), k


def two_instances(h, w, F, seed):
  """Two overlapping instances of objects 2 and 1 on h x w pixels, with masks."""
  rng = np.random.RandomState(seed)
  depth = np.zeros((2, h, w), np.float32)
  depth[0, :h - 1, :w - 2] = rng.uniform(500, 900, (h - 1, w - 2))
  depth[1, 1:, 2:] = rng.uniform(500, 900, (h - 1, w - 2))
  lp = (rng.uniform(-90, 90, (2, h, w, 3)) * (depth[..., None] > 0)).astype(np.float32)
  masks = (depth > 0).astype(np.uint8)
  masks[0, 2, 2] = 0                                     # rendered, but masked out
  centers = rng.uniform(-80, 80, (2, F, 3))
  sizes = rng.uniform(5, 40, (2, F))
  return depth, lp, masks, [2, 1], centers, sizes


@pytest.mark.parametrize('knn', [1, 2, 4])
@pytest.mark.parametrize('use_masks', [True, False])
def test_gt_fields_two_instances(knn, use_masks):
  depth, lp, masks, ids, centers, sizes = two_instances(5, 7, 4, seed=knn)
  masks = masks if use_masks else None
  got = run_gt(depth, lp, masks, ids, centers, sizes, knn)
  same_fields(got, knn_ref.gt_fields(depth, lp, masks, ids, centers, sizes, knn))
  fg = got['obj_label'] > 0
  assert fg.any() and not fg.all()
  if knn == 4:                                           # k == F: every fragment, sorted
    assert (np.sort(got['frag_label'][fg], axis=1) == np.arange(4)).all()
  if knn == 1:                                           # the old entry: the same bytes
    old = run_gt(depth, lp, masks, ids, centers, sizes, 1, old=True)
    for k in got:
      assert got[k].tobytes() == old[k].tobytes(), k


def test_gt_fields_planted_tie():
  # two centres equidistant from the pixel, in every position of the order: the lower index first
  centers = np.array([[[0.0, 0, 2.0], [1.0, 0, 0], [-1.0, 0, 0], [0, 3.0, 0], [0, -3.0, 0]]])
  sizes = np.array([[2.0, 4.0, 8.0, 16.0, 32.0]])
  depth = np.ones((1, 1, 3), np.float32)
  lp = np.zeros((1, 1, 3, 3), np.float32)
  lp[0, 0, 1] = [0.0, 0.0, 2.0]                          # at centre 0: then 1 and 2 tie
  lp[0, 0, 2] = [0.0, 0.0, -6.0]
  for knn in (1, 2, 3, 4):
    got = run_gt(depth, lp, None, [1], centers, sizes, knn)
    same_fields(got, knn_ref.gt_fields(depth, lp, None, [1], centers, sizes, knn))
    assert got['frag_label'][0, 0].tolist() == [1, 2, 0, 3][:knn]
    assert got['frag_label'][0, 1].tolist() == [0, 1, 2, 3][:knn]


def test_gt_fields_f256_and_the_fixture_points():
  depth, lp, masks, ids, centers, sizes = two_instances(6, 9, 256, seed=9)
  got = run_gt(depth, lp, masks, ids, centers, sizes, 4)
  same_fields(got, knn_ref.gt_fields(depth, lp, masks, ids, centers, sizes, 4))
  # the reference's own assignment: the fixture's points as a 20 x 25 local_pos image
  g = np.load(GOLDEN)
  lp = g['xyz'].reshape(1, 20, 25, 3)
  depth = np.ones((1, 20, 25), np.float32)
  for knn in (1, 2, 3, 4):
    got = run_gt(depth, lp, None, [1], g['centers'][None], g['sizes'][None], knn)
    assert got['frag_label'].reshape(500, knn).tobytes() == g['ids_k%d' % knn].tobytes()
    assert got['frag_loc'].reshape(500, knn, 3).tobytes() == g['coords_k%d' % knn].tobytes()
    assert (got['frag_weight'] == 1).all() and (got['obj_label'] == 1).all()


def test_gt_fields_refusals():
  lib = _lib()
  depth, lp, masks, ids, centers, sizes = two_instances(5, 7, 4, seed=1)
  t = [torch.zeros(8, device='cuda') for _ in range(4)]
  for knn in (0, 5, -1):
    assert lib.epos_gt_fields_knn(_p(t[0]), _p(t[1]), None, _p(t[2]), 1, 1, 1, _p(t[3]), _p(t[3]),
                                  2, 8, knn, None, None, None, None, None, None) == INVALID
  assert lib.epos_gt_fields_knn(_p(t[0]), _p(t[1]), None, _p(t[2]), 1, 1, 1, _p(t[3]), _p(t[3]),
                                2, 3, 4, None, None, None, None, None, None) == INVALID     # k > F
  assert lib.epos_last_error() == (b'epos_gt_fields_knn: knn must be in 1..min(num_frags, '
                                   b'EPOS_LOSS_MAX_KNN)')


# ------------------------------------------------------------------ the loss family ---
class Dev(object):
  """A knn_ref.make_case case on the device; every entry of the family over it. old=True calls
  the entry without knn (knn == 1 only)."""

  def __init__(self, c, ld_obj=None, offsets=(0, 0, 0), ignore=IGNORE):
    self.c, self.ignore = c, ignore
    self.B, self.P, O1 = c['obj_logits'].shape
    self.O, self.F = c['frag_logits'].shape[2:4]
    self.knn = c['gt_frag'].shape[2]
    self.ld_obj = O1 if ld_obj is None else ld_obj
    padded = np.full((self.B * self.P, self.ld_obj), np.nan, np.float32)   # never read
    padded[:, :O1] = c['obj_logits'].reshape(-1, O1)
    self.obj = _off(padded, offsets[0])
    self.frag = _off(c['frag_logits'], offsets[1])
    self.loc = _off(c['frag_loc'], offsets[2])
    self.g_obj = torch.from_numpy(np.ascontiguousarray(c['gt_obj'], np.int32)).cuda()
    self.g_frag = torch.from_numpy(np.ascontiguousarray(c['gt_frag'], np.int32)).cuda()
    self.g_loc = torch.from_numpy(np.ascontiguousarray(c['gt_loc'], np.float32)).cuda()
    self.g_w = torch.from_numpy(np.ascontiguousarray(c['gt_weight'], np.float32)).cuda()

  def head(self, old):
    """The arguments the entries share, up to ignore_label (and knn)."""
    a = (_p(self.obj), self.ld_obj, _p(self.frag), _p(self.loc), _p(self.g_obj), _p(self.g_frag),
         _p(self.g_loc), _p(self.g_w), self.B, self.P, self.O, self.F, self.ignore)
    if old:
      assert self.knn == 1
      return a
    return a + (self.knn,)

  def terms(self, old=False):
    lib = _lib()
    B, O1 = self.B, self.O + 1
    nbytes = lib.epos_loss_workspace_bytes(B, self.P, self.O, self.F)
    assert nbytes > 0, lib.epos_last_error()
    ws = torch.full((nbytes // 8,), -7, dtype=torch.int64, device='cuda')
    out = (torch.full((B, O1, 3), -7.0, dtype=torch.float64, device='cuda'),
           torch.full((B, O1, 2), -7, dtype=torch.int64, device='cuda'),
           torch.full((B,), -7, dtype=torch.int64, device='cuda'))
    fn = lib.epos_loss_terms if old else lib.epos_loss_terms_knn
    rc = fn(*self.head(old), _p(ws), _p(out[0]), _p(out[1]), _p(out[2]), _stream())
    assert rc == 0, lib.epos_last_error()
    torch.cuda.synchronize()
    self.tables = out
    return tuple(t.cpu().numpy() for t in out)

  def reduce(self, reduction, old=False):
    """(values f64 [4], scales f64 [B,3]) of the tables terms() left on the device."""
    lib = _lib()
    values = torch.full((4,), -7.0, dtype=torch.float64, device='cuda')
    scales = torch.full((self.B, 3), -7.0, dtype=torch.float64, device='cuda')
    a = (_p(self.tables[0]), _p(self.tables[1]), self.B, self.O) + WEIGHTS + (reduction,)
    if old:
      rc = lib.epos_loss_reduce(*a, _p(values), _p(scales), _stream())
    else:
      rc = lib.epos_loss_reduce_knn(*a, self.knn, _p(values), _p(scales), _stream())
    assert rc == 0, lib.epos_last_error()
    torch.cuda.synchronize()
    return values.cpu().numpy(), scales.cpu().numpy()

  def scales_upstream(self, scales, upstream):
    sc = torch.from_numpy(np.ascontiguousarray(scales, np.float64)).cuda()
    up = None if upstream is None else torch.tensor(upstream, dtype=torch.float64, device='cuda')
    return sc, up

  def grads(self, scales, upstream=None, old=False):
    """(d_obj, d_frag, d_loc) as uint32 bits, shaped like the logits; every element written."""
    lib = _lib()
    n, O, F = self.B * self.P, self.O, self.F
    sc, up = self.scales_upstream(scales, upstream)
    d = [_out(n * m, off) for m, off in ((O + 1, 0), (O * F, 1), (O * F * 3, 2))]
    fn = lib.epos_loss_grads if old else lib.epos_loss_grads_knn
    rc = fn(*self.head(old), _p(sc), _p(up), _p(d[0]), O + 1, _p(d[1]), _p(d[2]), _stream())
    assert rc == 0, lib.epos_last_error()
    torch.cuda.synchronize()
    self.d = d
    bits = [_bits(t) for t in d]
    for b in bits:
      assert not (b == SENTINEL).any()
    return (bits[0].reshape(self.B, self.P, O + 1), bits[1].reshape(self.B, self.P, O, F),
            bits[2].reshape(self.B, self.P, O, F, 3))

  def wgrad(self, A_padded, K, scales, upstream=None, old=False):
    """{(head, j): uint32 bits} of the six outputs."""
    lib = _lib()
    B, P, O, F = self.B, self.P, self.O, self.F
    sc, up = self.scales_upstream(scales, upstream)
    A = _off(A_padded, 0)
    nbytes = lib.epos_heads_wgrad_workspace_bytes(B, P, O, F, K)
    assert nbytes >= 20 * B * P, lib.epos_last_error()
    ws = torch.full((nbytes // 8 + 1,), -1, dtype=torch.int64, device='cuda')
    widths = {'obj': O + 1, 'frag': O * F, 'loc': O * F * 3}
    keys = [(h, j) for h in heads_wgrad_ref.HEADS for j in (0, 1)]
    bufs = [_out((K if j == 0 else 1) * widths[h], 0) for h, j in keys]
    fn = lib.epos_heads_wgrad_f32 if old else lib.epos_heads_wgrad_knn_f32
    rc = fn(_p(A), A_padded.shape[1], K, *self.head(old), _p(sc), _p(up), _p(ws),
            *[_p(b) for b in bufs], _stream())
    assert rc == 0, lib.epos_last_error()
    torch.cuda.synchronize()
    got = {}
    for key, b in zip(keys, bufs):
      raw = _bits(b)
      assert not (raw == SENTINEL).any(), key
      got[key] = raw.reshape(K, -1) if key[1] == 0 else raw
    return got

  def dgrad(self, Ws, K, scales, upstream=None, Y=None, old=False, ldx=None):
    """dX as uint32 bits [B*P, K]; Ws = the three matrices [K, N] in the checkpoint layout."""
    lib = _lib()
    n = self.B * self.P
    sc, up = self.scales_upstream(scales, upstream)
    wt = [torch.from_numpy(np.ascontiguousarray(w.T, np.float32)).cuda() for w in Ws]
    y = None if Y is None else torch.from_numpy(np.ascontiguousarray(Y, np.float32)).cuda()
    ldx = K if ldx is None else ldx
    dx = _out(n * ldx, 0)
    fn = lib.epos_heads_dgrad_f32 if old else lib.epos_heads_dgrad_knn_f32
    rc = fn(*self.head(old), _p(sc), _p(up), _p(wt[0]), _p(wt[1]), _p(wt[2]), K, K, _p(y), K,
            _p(dx), ldx, _stream())
    assert rc == 0, lib.epos_last_error()
    torch.cuda.synchronize()
    raw = _bits(dx).reshape(n, ldx)
    assert not (raw[:, :K] == SENTINEL).any() and (raw[:, K:] == SENTINEL).all()
    return raw[:, :K]


def take(c, images):
  return {k: np.ascontiguousarray(v[list(images)]) for k, v in c.items()}


def check_terms(got, exp, O, F, knn):
  """Counts, bad, zeros and the localisation sums exactly; the cross-entropy sums within
  loss_ref.ce_bound with the number of (pixel, slot) rows for n."""
  (sums, counts, bad), (e_sums, e_counts, e_bad) = got, exp
  assert counts.tobytes() == e_counts.tobytes() and bad.tobytes() == e_bad.tobytes()
  assert sums[:, :, 2].tobytes() == e_sums[:, :, 2].tobytes()
  assert not sums[:, 0, 1:].view(np.uint64).any()          # background: +0.0
  for k, (row_len, rows) in enumerate(zip(loss_ref.row_lengths(O, F), (1, knn))):
    for b in range(sums.shape[0]):
      for g in range(O + 1):
        ref, n = e_sums[b, g, k], int(e_counts[b, g, 0]) * rows
        print('ce b %d g %d k %d: err %.3g bound %.3g' % (
            b, g, k, abs(sums[b, g, k] - ref), loss_ref.ce_bound(row_len, n, ref)))
        assert abs(sums[b, g, k] - ref) <= loss_ref.ce_bound(row_len, n, ref), (b, g, k)


def check_grads(got, c, scales, upstream, O, F, knn):
  """Zeros and the localisation gradient exactly; the softmax gradients within the bound."""
  exp = knn_ref.grads(c, scales, upstream)
  masks = knn_ref.active_masks(c)
  u = loss_grad_ref.upstream_factors(upstream)
  for bits, m in zip(got, masks):
    assert not bits[~m].any()                               # +0.0 bytes
  assert got[2].tobytes() == exp[2].view(np.uint32).tobytes()
  for k, row_len, mult in ((0, O + 1, 1), (1, F, knn)):
    val, ref = got[k].view(np.float32).astype(np.float64), exp[k].astype(np.float64)
    for b in range(val.shape[0]):
      tol = knn_ref.softmax_bound(exp[k][b], float(scales[b, k]) * u[k], row_len, mult)
      err = np.abs(val[b] - ref[b])
      print('head %d image %d: worst error / bound %.3f' % (k, b, float((err / tol).max())))
      assert (err <= tol).all(), (k, b)


def loss_round(c, O, F, knn, ld_obj=None, offsets=(0, 0, 0), reduction=MEAN, upstream=None):
  """terms, reduce and grads of one case against knn_ref and loss.summarize; the old entries at
  k = 1; every image alone against its position in the batch."""
  from epos_amd import loss
  lib = _lib()
  B, P = c['gt_obj'].shape
  share = int(lib.epos_loss_share_pixels(P, O, F))
  dev = Dev(c, ld_obj, offsets)
  got = dev.terms()
  exp = knn_ref.terms(c, share)
  check_terms(got, exp, O, F, knn)
  values, scales = dev.reduce(reduction)
  if not exp[2].any():
    host = loss.summarize(got[0], got[1], got[2], WEIGHTS, O, knn)
    want = host['mean' if reduction == MEAN else 'pooled']
    assert values.tolist() == [want[n] for n in loss.NAMES]
  assert scales.tobytes() == knn_ref.scales(got[1], WEIGHTS, reduction, knn).tobytes()
  d = dev.grads(scales, upstream)
  check_grads(d, c, scales, upstream, O, F, knn)
  if knn == 1:
    for a, b in zip(dev.terms(old=True), got):
      assert a.tobytes() == b.tobytes()
    v_old, s_old = dev.reduce(reduction, old=True)
    assert v_old.tobytes() == values.tobytes() and s_old.tobytes() == scales.tobytes()
    for a, b in zip(dev.grads(scales, upstream, old=True), d):
      assert a.tobytes() == b.tobytes()
  if B > 1:
    for b in range(B):
      one = Dev(take(c, [b]), ld_obj, offsets)
      for x, y in zip(one.terms(), got):
        assert x[0].tobytes() == y[b].tobytes()
      for x, y in zip(one.grads(scales[b:b + 1], upstream), d):
        assert x[0].tobytes() == y[b].tobytes()
  return dev, scales


@pytest.mark.parametrize('O', [1, 3])
@pytest.mark.parametrize('F,knn', [(F, k) for F in (1, 4, 5, 64, 256) for k in (1, 2, 4)
                                   if k <= F])
def test_loss_sweep(F, knn, O):
  """Lane counts L = 1, 1, 2, 16, 64; k = 1, 2, 4 with k <= F; P = 1, 63, 65 around the share;
  B = 3 with every image alone; both reductions, with and without upstream, in turn."""
  for i, P in enumerate((1, 63, 65)):
    reduction, upstream = ((MEAN, UPSTREAM), (POOLED, None), (MEAN, None), (POOLED, UPSTREAM))[
        (i + knn + O) % 4]
    c = knn_ref.make_case(3, P, O, F, knn, seed=1000 * F + 10 * O + knn + P, empty_images=(1,))
    loss_round(c, O, F, knn, reduction=reduction, upstream=upstream)


@pytest.mark.parametrize('knn', [1, 2, 4])
def test_loss_odd_row_stride_and_offsets(knn):
  # ld_obj odd and the fragment heads off the 16-byte boundary: the non-vector paths
  O, F, P = 3, 8, 65
  c = knn_ref.make_case(2, P, O, F, knn, seed=77 + knn)
  base, _ = loss_round(c, O, F, knn)
  other, _ = loss_round(c, O, F, knn, ld_obj=O + 2, offsets=(1, 1, 3))
  for a, b in zip(base.terms(), other.terms()):
    assert a.tobytes() == b.tobytes()


PLANTS = [('gt_obj', (0, 9), 4), ('gt_frag', (0, 9, 0), 8), ('gt_frag', (0, 9, 1), -1),
          ('gt_weight', (0, 9, 1), 0.0), ('gt_weight', (0, 9, 0), np.inf),
          ('gt_weight', (0, 9, 1), np.nan), ('gt_weight', (0, 9, 0), -1.0),
          ('gt_frag', (0, 9, 1), 'first')]


@pytest.mark.parametrize('plant', range(len(PLANTS)))
def test_bad_pixel_rules(plant):
  """One planted pixel per bad rule, the three new ones included (a second slot outside the
  fragments, a second slot's weight, two slots naming one fragment)."""
  O, F, P, knn = 3, 8, 20, 2
  c = knn_ref.make_case(1, P, O, F, knn, seed=5, ignore_band=False)
  c['gt_obj'][0, 9] = 2
  c['gt_frag'][0, 9] = [3, 6]
  c['gt_weight'][0, 9] = [1.0, 0.5]
  assert Dev(c).terms()[2][0] == 0
  key, at, value = PLANTS[plant]
  c[key][at] = c['gt_frag'][0, 9, 0] if value == 'first' else value
  dev, scales = loss_round(c, O, F, knn)
  sums, counts, bad = dev.terms()
  assert bad[0] == 1
  assert not any(b[0, 9].any() for b in dev.grads(scales))


# ------------------------------------------------------------------ weight gradient ---
def features(n_pix, K, seed, lda=None):
  rng = np.random.RandomState(seed)
  A = (1.5 * rng.randn(n_pix, K)).astype(np.float32)
  A[rng.rand(n_pix, K) < 0.3] = 0.0
  padded = np.full((n_pix, K if lda is None else lda), np.nan, np.float32)
  padded[:, :K] = A
  return A, padded


def check_wgrad(dev, got, A, scales, upstream):
  """Against knn_ref.wgrads on the device's own epos_loss_grads_knn output, to the bound;
  columns nobody adds to are +0.0 bytes."""
  B, P, O, F = dev.B, dev.P, dev.O, dev.F
  d = [b.view(np.float32) for b in dev.grads(scales, upstream)]
  cls, frag = knn_ref.classes(dev.c)
  sums, abs_sums, n_terms = knn_ref.wgrads(A, d[0].reshape(B * P, O + 1),
                                           d[1].reshape(B * P, O, F),
                                           d[2].reshape(B * P, O, F, 3), cls, frag)
  worst = 0.0
  for (h, j), bits in got.items():
    assert not bits[..., n_terms[h] == 0].any(), (h, j)
    ok, w = heads_wgrad_ref.within(bits.view(np.float32), sums[h][j], abs_sums[h][j], n_terms[h])
    assert ok, (h, j, w)
    worst = max(worst, w)
  return worst


@pytest.mark.parametrize('knn', [1, 2, 4])
@pytest.mark.parametrize('F,K,P', [(4, 1, 400), (4, 17, 65), (128, 17, 200), (256, 1, 100),
                                   (256, 17, 33), (4, 8, 2048)])
def test_wgrad_sweep(F, K, P, knn):
  """K = 1, 17: the slice remainder and the bias row; F = 4, 128, 256: slices of 16, 8, 4
  feature indices and batches of 64, 32, 16 pixels, with more pixels of one class than a batch;
  K = 8, P = 2048: two ranges and the closing pass."""
  lib = _lib()
  O, B = 2, 2
  R = 2 if P == 2048 else 1
  assert lib.epos_heads_wgrad_range_pixels(P, O, F, K) == P // R
  c = knn_ref.make_case(B, P, O, F, knn, seed=F + K + P + knn)
  dev = Dev(c)
  A, padded = features(B * P, K, seed=P + knn, lda=K + 3)
  counts = dev.terms()[1]
  if P >= 100:                                              # more than one batch of a class
    assert counts[:, 1:, 0].max() > min(64, 4096 // F)
  scales = knn_ref.scales(counts, WEIGHTS, POOLED, knn)
  got = dev.wgrad(padded, K, scales, UPSTREAM)
  print('F %d K %d P %d knn %d: worst error / bound %.3f' % (
      F, K, P, knn, check_wgrad(dev, got, A, scales, UPSTREAM)))
  again = dev.wgrad(padded, K, scales, UPSTREAM)
  for key in got:
    assert got[key].tobytes() == again[key].tobytes(), key
  if knn == 1:
    old = dev.wgrad(padded, K, scales, UPSTREAM, old=True)
    for key in got:
      assert got[key].tobytes() == old[key].tobytes(), key


def integer_case(B, P, O, F, knn, seed):
  """A case whose every logit gradient and product is exact: equal logits in every row (O+1 and
  F powers of two), integer localisation differences, weights 1 and 2."""
  c = knn_ref.make_case(B, P, O, F, knn, seed, ignore_band=True)
  rng = np.random.RandomState(seed)
  c['obj_logits'][:] = 0.0
  c['frag_logits'][:] = 0.0
  c['frag_loc'] = rng.randint(-3, 4, c['frag_loc'].shape).astype(np.float32)
  c['gt_loc'] = rng.randint(-3, 4, c['gt_loc'].shape).astype(np.float32)
  c['gt_weight'] = np.where(c['gt_weight'] > 0, rng.randint(1, 3, c['gt_weight'].shape),
                            0).astype(np.float32)
  return c


@pytest.mark.parametrize('knn', [1, 2, 4])
@pytest.mark.parametrize('F,K,P', [(4, 17, 200), (128, 1, 70), (256, 17, 40), (4, 8, 2048)])
def test_wgrad_and_dgrad_bit_equal_on_exact_data(F, K, P, knn):
  """Every term is a small dyadic number, so every order of summation gives the exact sum: the
  device equals the restatement bit for bit."""
  O, B = 3, 2
  c = integer_case(B, P, O, F, knn, seed=F + P + knn)
  dev = Dev(c)
  rng = np.random.RandomState(knn)
  A = rng.randint(-4, 5, (B * P, K)).astype(np.float32)
  scales = np.tile(np.array([[0.5, 0.25, 2.0]]), (B, 1))
  got = dev.wgrad(A, K, scales)
  d = knn_ref.grads(c, scales)
  assert dev.grads(scales)[1].tobytes() == d[1].view(np.uint32).tobytes()
  cls, frag = knn_ref.classes(c)
  sums, _, _ = knn_ref.wgrads(A, d[0].reshape(B * P, -1), d[1].reshape(B * P, O, F),
                              d[2].reshape(B * P, O, F, 3), cls, frag)
  for (h, j), bits in got.items():
    assert bits.tobytes() == np.asarray(sums[h][j], np.float32).view(np.uint32).tobytes(), (h, j)
  Ws = [rng.randint(-2, 3, (K, n)).astype(np.float32) for n in (O + 1, O * F, O * F * 3)]
  dx, _, _ = knn_ref.dgrad(*d, *Ws, cls, frag)
  assert dev.dgrad(Ws, K, scales).tobytes() == dx.astype(np.float32).view(np.uint32).tobytes()


# ------------------------------------------------------------------ input gradient ---
@pytest.mark.parametrize('knn', [1, 2, 4])
@pytest.mark.parametrize('K,O,F,relu', [(3, 2, 5, False), (256, 2, 8, True), (260, 3, 4, True),
                                        (8, 70, 4, False), (12, 2, 130, True)])
def test_dgrad_sweep(K, O, F, relu, knn):
  """K = 3: the scalar path; 256, 260: 16 bytes per lane; O + 1 > 64 and F > 64: two column
  chunks; with and without the ReLU mask. The bound is heads_dgrad_ref's, n_active = O+1 + F +
  3 knn for a foreground pixel."""
  B, P = 2, 37
  c = knn_ref.make_case(B, P, O, F, knn, seed=K + O + F + knn)
  dev = Dev(c)
  counts = dev.terms()[1]
  scales = knn_ref.scales(counts, WEIGHTS, MEAN, knn)
  rng = np.random.RandomState(K)
  Ws = [(0.5 * rng.randn(K, n)).astype(np.float32) for n in (O + 1, O * F, O * F * 3)]
  Y = rng.randn(B * P, K).astype(np.float32) if relu else None
  if relu:
    Y[::3, ::2] = -0.0
  got = dev.dgrad(Ws, K, scales, UPSTREAM, Y)
  d = [b.view(np.float32) for b in dev.grads(scales, UPSTREAM)]
  cls, frag = knn_ref.classes(c)
  sums, abs_sums, n_active = knn_ref.dgrad(*d, *Ws, cls, frag)
  assert n_active.max() == O + 1 + F + 3 * knn and (n_active[cls < 0] == 0).all()
  ref = sums if Y is None else heads_dgrad_ref.relu_mask(sums, Y)
  ok, worst = heads_dgrad_ref.within(got.view(np.float32), ref, abs_sums, n_active)
  print('K %d O %d F %d knn %d: worst error / bound %.3f' % (K, O, F, knn, worst))
  assert ok
  assert not got[cls < 0].any()                             # zero rows: +0.0 bytes
  if Y is not None:
    assert not got[Y <= 0].any()                            # masked elements: +0.0 bytes
  # slots given in descending fragment order: the same bytes (the sum runs by column)
  order = np.argsort(-c['gt_frag'], axis=2, kind='stable')
  c2 = dict(c)
  c2['gt_frag'] = np.take_along_axis(c['gt_frag'], order, axis=2)
  c2['gt_weight'] = np.take_along_axis(c['gt_weight'], order, axis=2)
  c2['gt_loc'] = np.take_along_axis(c['gt_loc'], order[..., None], axis=2)
  assert Dev(c2).dgrad(Ws, K, scales, UPSTREAM, Y).tobytes() == got.tobytes()
  if knn == 1:
    assert dev.dgrad(Ws, K, scales, UPSTREAM, Y, old=True).tobytes() == got.tobytes()
