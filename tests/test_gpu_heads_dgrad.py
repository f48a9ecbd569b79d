"""epos_heads_dgrad_f32 on the device (csrc/heads_dgrad.hip) and the Python layer over it
(heads_train.heads_input_grad, net_feature_grad, loss.differentiable_losses_from_features). The
reference for the logit gradients d is the device's own epos_loss_grads output on the same
inputs (pinned by test_gpu_loss_grad.py), fed to tests/helpers/heads_dgrad_ref.py: the
comparison is about the fp64 sum over a pixel's active columns only, to heads_dgrad_ref.bound.
dX is pre-filled with a sentinel: every element must be written, zeros as +0.0 bytes, and the
padding columns untouched."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import (heads_dgrad_ref as ref, heads_wgrad_ref, loss_cases,      # noqa: E402
                           loss_device, loss_grad_ref)
from tests.helpers.loss_device import (IGNORE, KEYS, MEAN, NET_B, NET_F, NET_H,   # noqa: E402,F401
                                       NET_O, NET_W, POOLED, SENTINEL, UPSTREAM, WEIGHTS, _lib,
                                       _p, _stream, gt_tensors, net_logits, ref_counts,
                                       small_net, tensors)

pytestmark = pytest.mark.gpu

INVALID = -1                               # EPOS_E_INVALID


def _dev(a, dtype=torch.float32):
  return torch.from_numpy(np.ascontiguousarray(a)).to(device='cuda', dtype=dtype)


def _padded(a, ld):
  """a [rows, n] in a NaN-filled [rows, ld]: the padding is never read."""
  out = np.full((a.shape[0], ld), np.nan, np.float32)
  out[:, :a.shape[1]] = a
  return out


def head_matrices(O, F, K, seed):
  """The three weight matrices in the checkpoint layout, f32 [K, N]."""
  rng = np.random.RandomState(seed)
  return [(0.5 * rng.randn(K, n)).astype(np.float32) for n in (O + 1, O * F, O * F * 3)]


class Device(object):
  """A host case and the weights on the device, with the logit gradients epos_loss_grads writes
  for it. pad = extra columns of the object logits (ld_obj) and of the transposed weights
  (ldwt)."""

  def __init__(self, c, Ws, scale, upstream=None, pad=(0, 0), ignore=IGNORE):
    self.c, self.Ws, self.ignore = c, Ws, ignore
    self.B, self.P, O1 = c['obj_logits'].shape
    self.O, self.F = c['frag_logits'].shape[2:4]
    self.K = Ws[0].shape[0]
    self.n = self.B * self.P
    self.ld_obj, self.ldwt = O1 + pad[0], self.K + pad[1]
    self.obj = _dev(_padded(c['obj_logits'].reshape(self.n, O1), self.ld_obj))
    self.frag, self.loc = _dev(c['frag_logits']), _dev(c['frag_loc'])
    self.g_obj = _dev(np.asarray(c['gt_obj'], np.int32), torch.int32)
    self.g_frag = _dev(np.asarray(c['gt_frag'], np.int32), torch.int32)
    self.g_loc = _dev(np.asarray(c['gt_loc'], np.float32))
    self.g_w = _dev(np.asarray(c['gt_weight'], np.float32))
    self.sc = _dev(np.ascontiguousarray(scale, np.float64), torch.float64)
    self.up = None if upstream is None else torch.tensor(upstream, dtype=torch.float64,
                                                         device='cuda')
    self.wt = [_dev(_padded(np.ascontiguousarray(W.T), self.ldwt)) for W in Ws]
    self._ref = None

  def logit_grads(self):
    return loss_device.logit_grads(self)

  def reference(self):
    """(sums, abs_sums, n_active) of heads_dgrad_ref.dgrad on the device's own d, computed once."""
    if self._ref is None:
      d = [t.cpu().numpy() for t in self.logit_grads()]
      cls, frag = heads_wgrad_ref.classes(self.c, self.ignore)
      self._ref = ref.dgrad(d[0].reshape(self.n, -1), d[1].reshape(self.n, self.O, self.F),
                            d[2].reshape(self.n, self.O, self.F, 3), *self.Ws, cls, frag)
    return self._ref

  def call(self, dX, ldx, Y=None, ldy=0, B=None, P=None, K=None, O=None, F=None, ld_obj=None,
           ldwt=None, null=()):
    """The raw call; `null` names pointers passed as NULL."""
    lib = _lib()
    ptr = {'obj': self.obj, 'frag': self.frag, 'loc': self.loc, 'g_obj': self.g_obj,
           'g_frag': self.g_frag, 'g_loc': self.g_loc, 'g_w': self.g_w, 'sc': self.sc,
           'up': self.up, 'wt0': self.wt[0], 'wt1': self.wt[1], 'wt2': self.wt[2], 'dX': dX}
    a = {k: (None if k in null else _p(v)) for k, v in ptr.items()}
    return lib.epos_heads_dgrad_f32(
        a['obj'], self.ld_obj if ld_obj is None else ld_obj, a['frag'], a['loc'], a['g_obj'],
        a['g_frag'], a['g_loc'], a['g_w'], self.B if B is None else B,
        self.P if P is None else P, self.O if O is None else O, self.F if F is None else F,
        self.ignore, a['sc'], a['up'], a['wt0'], a['wt1'], a['wt2'],
        self.ldwt if ldwt is None else ldwt, self.K if K is None else K, _p(Y), ldy, a['dX'], ldx,
        _stream())

  def run(self, Y=None, ldy=0, pad_x=0):
    """One call. Returns the uint32 bits of dX [B*P, K]; the padding must keep the sentinel."""
    ldx = self.K + pad_x
    buf = torch.full((self.n, ldx), SENTINEL, dtype=torch.int32, device='cuda')
    rc = self.call(buf.view(torch.float32), ldx, Y, ldy)
    assert rc == 0, _lib().epos_last_error()
    torch.cuda.synchronize()
    raw = buf.cpu().numpy().view(np.uint32)
    assert (raw[:, self.K:] == SENTINEL).all()               # the padding is not touched
    assert not (raw[:, :self.K] == SENTINEL).any()           # every element is written
    return np.ascontiguousarray(raw[:, :self.K])

  def check(self, bits, Y=None):
    """dX against the reference, to bound; rows nobody adds to and masked elements are +0.0
    bytes. Returns the worst error / bound."""
    sums, abs_sums, n_active = self.reference()
    if Y is not None:
      masked = ~(Y > 0) & ~np.isnan(Y)
      assert masked.any() and not bits[masked].any()         # +0.0, not -0.0
      sums, abs_sums = ref.relu_mask(sums, Y), ref.relu_mask(abs_sums, Y)
    assert not bits[n_active == 0].any()
    ok, worst = ref.within(bits.view(np.float32), sums, abs_sums, n_active)
    assert ok, worst
    return worst

  def check_dense(self, bits):
    """The same bound against torch's fp64 d @ W^T of the device's d, on the device."""
    d = self.logit_grads()
    dense = sum(t.view(self.n, -1).double() @ _dev(W).double().t() for t, W in zip(d, self.Ws))
    _, abs_sums, n_active = self.reference()
    ok, worst = ref.within(bits.view(np.float32), dense.cpu().numpy(), abs_sums, n_active)
    assert ok, worst


def make(B, P, O, F, K, seed, reduction=MEAN, upstream=None, pad=(0, 0), empty_images=(),
         edit=None, edit_w=None):
  c = loss_cases.make_case(B, P, O, F, seed, empty_images=empty_images)
  Ws = head_matrices(O, F, K, seed + 1)
  if edit is not None:
    edit(c)
  if edit_w is not None:
    edit_w(Ws)
  scale = loss_grad_ref.scales(ref_counts(c), WEIGHTS, reduction)
  return Device(c, Ws, scale, upstream, pad)


# (O, F, K): the smallest head; odd sizes (one k per lane); a whole wave of fragments and one
# 16-byte group of k per lane; four chunks of 64 fragments; the C2 head; K = 1024, four 16-byte
# groups per lane (sixteen single k where a padding breaks the 16-byte rows); more than 64
# object columns, two chunks
SHAPES = [(1, 1, 1), (2, 3, 5), (3, 64, 256), (2, 256, 64), (21, 64, 256), (1, 2, 1024),
          (70, 2, 8)]


@pytest.mark.parametrize('O,F,K', SHAPES)
def test_sweep(O, F, K):
  # P through one pixel, a short and a long workgroup share (16 pixels, four waves): 63 and 65
  # leave a last workgroup of 15 pixels and of 1, 257 of 1 again after 16 full ones
  for i, P in enumerate([1, 63, 65, 257]):
    B = (1, 3)[i % 2]
    pad = ((0, 0), (3, 4), (1, 0), (0, 3))[(i + K) % 4]      # ld_obj, ldwt; 4 keeps 16-byte rows
    pad_x = (0, 4, 3, 0)[(i + O) % 4]
    reduction, upstream = ((MEAN, UPSTREAM), (POOLED, None), (MEAN, None), (POOLED, UPSTREAM))[
        (i + O) % 4]
    dev = make(B, P, O, F, K, seed=1000 * F + 10 * O + i, reduction=reduction,
               upstream=upstream, pad=pad, empty_images=(1,) if B > 1 else ())
    bits = dev.run(pad_x=pad_x)
    worst = dev.check(bits)
    dev.check_dense(bits)
    print('O %d F %d K %d P %d B %d pad %s %d: worst error / bound %.3f' % (
        O, F, K, P, B, pad, pad_x, worst))


def test_many_workgroups():
  # P = 1200: 75 workgroups per image, three images
  dev = make(3, 1200, 3, 64, 64, seed=41, reduction=POOLED, upstream=UPSTREAM, pad=(1, 4))
  bits = dev.run(pad_x=4)
  dev.check(bits)
  dev.check_dense(bits)


def test_images_of_one_class():
  O, F, K, P = 3, 6, 12, 70

  def edit(c):
    c['gt_obj'][0] = IGNORE
    c['gt_obj'][1] = 0
    c['gt_obj'][2] = 2
    fg = c['gt_obj'] == 2
    c['gt_frag'][:] = np.where(fg, np.abs(c['gt_frag']), -1)
    c['gt_weight'][:] = np.where(fg, np.maximum(c['gt_weight'], 0.25), 0.0)
    c['obj_logits'][0] = np.nan                              # an ignored pixel is not read
    c['frag_logits'][0] = np.inf
  dev = make(3, P, O, F, K, seed=42, edit=edit)
  bits = dev.run()
  dev.check(bits)
  n_active = dev.reference()[2].reshape(3, P)
  assert (n_active[0] == 0).all() and (n_active[1] == O + 1).all()
  assert (n_active[2] == O + 1 + F + 3).all()
  rows = bits.reshape(3, P, K)
  assert not rows[0].any() and rows[1].all() and rows[2].all()


def test_ignored_and_bad_pixels_get_zero_rows():
  O, F, K, P = 3, 6, 9, 120

  def edit(c):
    g, f, w = c['gt_obj'][0], c['gt_frag'][0], c['gt_weight'][0]
    g[20], g[21] = -1, O + 1                               # labels outside 0..O
    g[22:28] = 2
    f[22], f[23] = -1, F                                   # fragment outside 0..F-1
    w[24], w[25], w[26], w[27] = 0.0, -1.0, np.nan, np.inf
    f[24:28] = 1
    for p in list(range(20, 28)) + list(np.nonzero(g == IGNORE)[0]):     # must never be read
      c['obj_logits'][0, p] = np.nan
      c['frag_logits'][0, p] = np.inf
      c['frag_loc'][0, p] = np.nan
  dev = make(2, P, O, F, K, seed=24, pad=(2, 3), edit=edit)
  cls = heads_wgrad_ref.classes(dev.c, IGNORE)[0]
  assert (cls[20:28] == -1).all()
  bits = dev.run(pad_x=3)
  dev.check(bits)
  assert not bits[cls < 0].any() and np.isfinite(bits.view(np.float32)).all()
  assert bits[cls >= 0].any(axis=1).all()


@pytest.mark.parametrize('where,value', [('obj', np.nan), ('frag', np.inf), ('frag', np.nan),
                                         ('loc', np.nan), ('weight', np.nan)])
def test_non_finite_value_marks_only_its_own_pixels(where, value):
  # every class in one image; a NaN object logit, an infinite fragment logit (inf - inf in the
  # softmax), ... at one foreground pixel: its row is non-finite, every other row keeps its bytes
  O, F, K, P = 3, 6, 9, 100
  c0 = loss_cases.make_case(1, P, O, F, 25)
  p = int(np.nonzero(c0['gt_obj'][0] == 2)[0][0])
  f = int(c0['gt_frag'][0, p])
  clean = make(1, P, O, F, K, seed=25).run()

  def edit(c):
    if where == 'obj':
      c['obj_logits'][0, p, 1] = value
    elif where == 'frag':
      c['frag_logits'][0, p, 1, (f + 1) % F] = value
    elif where == 'loc':
      c['frag_loc'][0, p, 1, f, 2] = value

  def edit_w(Ws):
    if where == 'weight':
      Ws[1][4, 1 * F + 2] = value                          # k = 4 of (object 2, fragment 2)
  dev = make(1, P, O, F, K, seed=25, edit=edit, edit_w=edit_w)
  bits = dev.run()
  dev.check(bits)                                          # non-finite where the reference is
  bad = ~np.isfinite(bits.view(np.float32))
  if where == 'weight':                                    # every pixel of object 2, at k = 4
    exp = np.zeros((P, K), bool)
    exp[dev.c['gt_obj'][0] == 2, 4] = True
    assert exp.any() and (bad == exp).all()
  else:
    assert bad[p].all() and not np.delete(bad, p, 0).any()
  assert (bits[~bad] == clean[~bad]).all()


def test_relu_mask():
  B, P, O, F = 2, 90, 3, 6
  for K, pad_y, pad_x in ((12, 0, 0), (12, 4, 4), (7, 2, 1)):
    dev = make(B, P, O, F, K, seed=43, upstream=UPSTREAM)
    rng = np.random.RandomState(44)
    Y = (1.5 * rng.randn(B * P, K)).astype(np.float32)
    Y[rng.rand(B * P, K) < 0.2] = 0.0
    Y[rng.rand(B * P, K) < 0.1] = -0.0
    Y[P - 1, 0] = np.nan                                     # a foreground pixel; not <= 0: kept
    assert (Y > 0).any() and (Y < 0).any() and np.signbit(Y[Y == 0]).any()
    assert (~np.signbit(Y[Y == 0])).any()
    plain = dev.run(pad_x=pad_x)
    dY = _dev(_padded(Y, K + pad_y))
    bits = dev.run(Y=dY, ldy=K + pad_y, pad_x=pad_x)
    dev.check(bits, Y)
    keep = (Y > 0) | np.isnan(Y)
    assert (bits[keep] == plain[keep]).all() and not bits[~keep].any()
    # dX == Y is refused and nothing is written
    before = dY.clone()
    assert dev.call(dY, K + pad_y, Y=dY, ldy=K + pad_y) == INVALID
    assert _lib().epos_last_error() == (b'epos_heads_dgrad_f32: the output buffer starts at an '
                                        b'input pointer')
    torch.cuda.synchronize()
    assert dY.view(torch.int32).equal(before.view(torch.int32))


def test_determinism_and_batch_position():
  B, P, O, F, K = 3, 150, 3, 64, 40
  dev = make(B, P, O, F, K, seed=26, upstream=UPSTREAM)
  a, b = dev.run(), dev.run()
  assert a.tobytes() == b.tobytes()
  dev.check(a)
  scale = dev.sc.cpu().numpy()
  rows = a.reshape(B, P, K)
  for i in range(B):
    one = {k: np.ascontiguousarray(v[i:i + 1]) for k, v in dev.c.items()}
    alone = Device(one, dev.Ws, scale[i:i + 1], UPSTREAM).run()
    assert alone.tobytes() == rows[i].tobytes(), i
    for pos in range(3):                                   # image i at every position of a batch
      order = [(i + j - pos) % B for j in range(B)]
      assert order[pos] == i
      c2 = {k: np.ascontiguousarray(v[order]) for k, v in dev.c.items()}
      got = Device(c2, dev.Ws, scale[order], UPSTREAM).run().reshape(B, P, K)
      assert got[pos].tobytes() == rows[i].tobytes(), (i, pos)


def test_upstream():
  dev = make(2, 77, 3, 5, 8, seed=45)
  none = dev.run()
  dev.check(none)
  dev.up = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64, device='cuda')
  assert dev.run().tobytes() == none.tobytes()
  dev.up = torch.tensor(UPSTREAM, dtype=torch.float64, device='cuda')
  dev._ref = None
  bits = dev.run()
  dev.check(bits)
  assert bits.tobytes() != none.tobytes()


@pytest.mark.parametrize('O,F', [(2, 3), (3, 5)])
def test_identity_weights_give_the_logit_gradients_themselves(O, F):
  # K = N = O+1 + 4*O*F and the three weight matrices the row blocks of the N x N identity:
  # dX[p, k] has exactly one non-zero term, so dX is [d_obj | d_frag | d_loc] of epos_loss_grads
  # on the same inputs, element for element (as fp32 values: a sum that starts at +0.0 turns a
  # -0.0 into +0.0). That holds only while both kernels round an element with the same
  # function. N = 27: one k per lane; N = 64: the 16-byte path. P = 19: one full share of 16
  # pixels and a tail of three.
  B, P, N = 2, 19, O + 1 + 4 * O * F

  def edit(c):
    fg = np.nonzero((c['gt_obj'][1] >= 1) & (c['gt_obj'][1] <= O))[0]
    c['gt_obj'][1, fg[0]] = O + 1                          # two bad pixels
    c['gt_weight'][1, fg[1]] = 0.0

  def edit_w(Ws):
    r0 = 0
    for W in Ws:
      W[:] = np.eye(N, dtype=np.float32)[:, r0:r0 + W.shape[1]]
      r0 += W.shape[1]
  dev = make(B, P, O, F, N, seed=60 + F, edit=edit, edit_w=edit_w)
  cls = heads_wgrad_ref.classes(dev.c, IGNORE)[0]
  assert (cls == 0).any() and (cls > 0).any()              # background, foreground,
  assert (dev.c['gt_obj'] == IGNORE).any()                 # ignored
  assert ((cls < 0) & (dev.c['gt_obj'].reshape(-1) != IGNORE)).sum() == 2      # and bad pixels
  got = dev.run().view(np.float32)
  d = np.concatenate([t.cpu().numpy().reshape(B * P, -1) for t in dev.logit_grads()], axis=1)
  assert d.shape == got.shape == (B * P, N)
  assert np.isfinite(d).all() and d[cls >= 0].any(axis=1).all() and not d[cls < 0].any()
  assert (got == d).all(), np.argwhere(got != d)[:5]


def test_refusals_leave_dx_untouched():
  dev = make(2, 30, 3, 5, 8, seed=46)
  O, F, K = dev.O, dev.F, dev.K
  Y = torch.ones((dev.n, K), device='cuda')
  buf = torch.full((dev.n, K), SENTINEL, dtype=torch.int32, device='cuda')
  dX = buf.view(torch.float32)
  for kwargs, msg in (({'B': -1}, b'B must be >= 0'),
                      ({'B': 65536}, b'B must be <= 65535'),
                      ({'P': -1}, b'P must be in 0..2^31'),
                      ({'P': 2 ** 31 + 1}, b'P must be in 0..2^31'),
                      ({'O': 0}, b'num_objs must be in 1..4095'),
                      ({'O': 4096}, b'num_objs must be in 1..4095'),
                      ({'F': 0}, b'num_frags must be in 1..256'),
                      ({'F': 257}, b'num_frags must be in 1..256'),
                      ({'B': 65535, 'P': 2 ** 31},
                       b'B * workgroups per image must be below 2^31'),
                      ({'K': 0}, b'K must be in 1..1024'),
                      ({'K': 1025}, b'K must be in 1..1024'),
                      ({'ldx': K - 1}, b'ldx must be >= K'),
                      ({'ldwt': K - 1}, b'ldwt must be >= K'),
                      ({'Y': Y, 'ldy': K - 1}, b'ldy must be >= K'),
                      ({'ld_obj': O}, b'ld_obj must be >= num_objs + 1'),
                      ({'null': ('obj',)}, b'null pointer'),
                      ({'null': ('loc',)}, b'null pointer'),
                      ({'null': ('g_w',)}, b'null pointer'),
                      ({'null': ('sc',)}, b'null pointer'),
                      ({'null': ('wt2',)}, b'null pointer'),
                      ({'dX': dev.frag}, b'the output buffer starts at an input pointer'),
                      ({'dX': dev.wt[0]}, b'the output buffer starts at an input pointer'),
                      ({'dX': Y, 'Y': Y, 'ldy': K},
                       b'the output buffer starts at an input pointer')):
    kwargs = dict(kwargs)
    out = kwargs.pop('dX', dX)
    before = out.clone()
    assert dev.call(out, kwargs.pop('ldx', K), **kwargs) == INVALID, kwargs
    assert _lib().epos_last_error() == b'epos_heads_dgrad_f32: ' + msg, kwargs
    torch.cuda.synchronize()
    assert out.view(torch.int32).equal(before.view(torch.int32)), kwargs
  assert (buf == SENTINEL).all()
  # no pixel: returns 0 and writes nothing, null pointers or not
  everything = ('obj', 'frag', 'loc', 'g_obj', 'g_frag', 'g_loc', 'g_w', 'sc', 'wt0', 'wt1',
                'wt2', 'dX')
  assert dev.call(dX, K, B=0) == 0 and dev.call(dX, K, P=0) == 0
  assert dev.call(dX, K, P=0, null=everything) == 0
  torch.cuda.synchronize()
  assert (buf == SENTINEL).all()


# ---------------------------------------------------------------- through Python ---
def variables(Ws, seed=0, device='cuda'):
  """{variable name: tensor} of the six logits variables in the checkpoint layout."""
  rng = np.random.RandomState(seed)
  out = {}
  for name, W in zip(KEYS, Ws):
    out['logits/%s/weights' % name] = torch.from_numpy(W).view(1, 1, W.shape[0], -1).to(device)
    out['logits/%s/biases' % name] = torch.from_numpy(
        (0.5 * rng.randn(W.shape[1])).astype(np.float32)).to(device)
  return out


def test_heads_input_grad_entry_and_graph_capture():
  from epos_amd import heads_train
  B, h, w, O, F, K = 2, 9, 11, 3, 8, 24
  dev = make(B, h * w, O, F, K, seed=31, upstream=UPSTREAM)
  exp = dev.run()
  logits, gt = tensors(dev.c, h, w)
  hw = variables(dev.Ws)
  up = torch.tensor(UPSTREAM, dtype=torch.float64, device='cuda')
  dX = heads_train.heads_input_grad(logits, gt, dev.sc, hw, upstream=up)
  assert dX.dtype == torch.float32 and tuple(dX.shape) == (B * h * w, K)
  assert dX.cpu().numpy().tobytes() == exp.tobytes()
  # host arrays as trainer.Optimizer.state() holds them; out as a view of a wider buffer; workspace
  state = {k: v.cpu().numpy() for k, v in hw.items()}
  wide = torch.full((B, h, w, K + 8), -7.0, device='cuda')
  ws = torch.empty(((O + 1 + 4 * O * F) * K + 5,), device='cuda')
  got = heads_train.heads_input_grad(logits, gt, dev.sc, state, upstream=up,
                                     out=wide[..., :K], workspace=ws)
  assert got.data_ptr() == wide.data_ptr() and tuple(got.shape) == (B, h, w, K)
  assert got.reshape(-1, K).cpu().numpy().tobytes() == exp.tobytes()
  assert (wide[..., K:] == -7.0).all()
  # the mask: the features themselves as relu_of
  feats = torch.randn((B, h, w, K), device='cuda')
  masked = heads_train.heads_input_grad(logits, gt, dev.sc, hw, upstream=up, relu_of=feats)
  keep = (feats > 0).reshape(-1, K)
  assert torch.equal(masked[keep], dX[keep]) and not masked[~keep].view(torch.int32).any()
  with pytest.raises(ValueError, match='workspace must be'):
    heads_train.heads_input_grad(logits, gt, dev.sc, hw, workspace=ws[:7])
  with pytest.raises(KeyError, match='pred_frag_loc/weights'):
    heads_train.heads_input_grad(logits, gt, dev.sc, {
        k: v for k, v in hw.items() if k != 'logits/pred_frag_loc/weights'})
  with pytest.raises(ValueError, match='relu_of holds'):
    heads_train.heads_input_grad(logits, gt, dev.sc, hw, relu_of=feats[:1])
  # captured in a graph and replayed: the same bytes
  side = torch.cuda.Stream()
  out = torch.full((B * h * w, K), -7.0, device='cuda')
  with torch.cuda.stream(side):                            # warm-up outside the capture
    heads_train.heads_input_grad(logits, gt, dev.sc, hw, upstream=up, out=out, workspace=ws)
  torch.cuda.synchronize()
  out.fill_(-7.0)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    heads_train.heads_input_grad(logits, gt, dev.sc, hw, upstream=up, out=out, workspace=ws)
  graph.replay()
  torch.cuda.synchronize()
  assert out.cpu().numpy().tobytes() == exp.tobytes()


def torch_total(X, hw, c, O, F, weights, up):
  """sum_k up_k loss_k of the pooled batch in torch fp64 from features X [B,P,K] and the six
  variables: features -> three 1x1 convolutions -> the losses of loss_ref's restatement."""
  from tests.test_loss_grad_host import torch_losses
  B, P = X.shape[0], X.shape[1]
  shapes = [(B, P, O + 1), (B, P, O, F), (B, P, O, F, 3)]
  lin = [(X @ hw['logits/%s/weights' % k].double().view(X.shape[2], -1) +
          hw['logits/%s/biases' % k].double()).reshape(s) for k, s in zip(KEYS, shapes)]
  losses = torch_losses(*lin, c, range(B), O, F, weights)
  total = (losses[0] + losses[1]) + losses[2]
  return up[0] * losses[0] + up[1] * losses[1] + up[2] * losses[2] + up[3] * total


def test_differentiable_losses_from_features():
  from epos_amd import heads_train, loss
  B, P, O, F, K = 1, 9, 2, 3, 5
  c = loss_cases.make_case(B, P, O, F, seed=51, ignore_band=False)
  Ws = head_matrices(O, F, K, 52)
  hw = {k: v.requires_grad_() for k, v in variables(Ws, seed=53).items()}
  rng = np.random.RandomState(54)
  X_host = rng.randn(B, P, K).astype(np.float32)
  feats = torch.from_numpy(X_host).cuda().requires_grad_()
  gt = gt_tensors(c, 3, 3)
  values, bad = loss.differentiable_losses_from_features(feats.view(B, 3, 3, K), hw, gt, WEIGHTS,
                                                         'pooled')
  assert values.dtype == torch.float64 and values.shape == (4,) and bad.tolist() == [0]
  with torch.no_grad():
    logits = loss.logits_from_features(feats, hw)
  v2, _ = loss.differentiable_losses(logits, gt, WEIGHTS, 'pooled')
  assert torch.equal(values.detach(), v2)                  # bit-equal on the same logits
  up = torch.tensor(UPSTREAM, dtype=torch.float64, device='cuda')
  (values * up).sum().backward()
  sums, counts, _ = loss.loss_terms(logits, gt)
  _, scales = loss.loss_values(sums, counts, WEIGHTS, 'pooled')
  dX = heads_train.heads_input_grad(logits, gt, scales, hw, upstream=up)
  assert feats.grad.shape == feats.shape
  assert feats.grad.reshape(-1, K).cpu().numpy().tobytes() == dX.cpu().numpy().tobytes()
  raw = heads_train.heads_weight_grads(feats.detach(), logits, gt, scales, upstream=up)
  for k in KEYS:
    wname, bname = heads_train.variable_names(k)
    assert hw[wname].grad.shape == hw[wname].shape
    assert hw[wname].grad.cpu().numpy().tobytes() == raw[k][0].cpu().numpy().tobytes(), k
    assert hw[bname].grad.cpu().numpy().tobytes() == raw[k][1].cpu().numpy().tobytes(), k
  # only what needs a gradient is computed
  frozen = {k: v.detach() for k, v in hw.items()}
  f2 = feats.detach().clone().requires_grad_()
  loss.differentiable_losses_from_features(f2, frozen, gt, WEIGHTS, 'pooled')[0][3].backward()
  assert f2.grad is not None
  # the sign and scale convention of scales and upstream: one central finite difference of the
  # torch fp64 restatement on the host. The device differentiates at fp32 logits that differ
  # from the fp64 ones by rounding: 1e-4 of the largest entry covers that many times over.
  hw64 = {k: v.detach().cpu() for k, v in hw.items()}
  X = torch.from_numpy(X_host).double().requires_grad_()
  torch_total(X, hw64, c, O, F, WEIGHTS, UPSTREAM).backward()
  auto = X.grad.numpy()
  p, k, eps = 4, 2, 1e-6
  Xp, Xm = torch.from_numpy(X_host).double(), torch.from_numpy(X_host).double()
  Xp[0, p, k] += eps
  Xm[0, p, k] -= eps
  fd = float(torch_total(Xp, hw64, c, O, F, WEIGHTS, UPSTREAM) -
             torch_total(Xm, hw64, c, O, F, WEIGHTS, UPSTREAM)) / (2 * eps)
  assert abs(fd - auto[0, p, k]) <= 1e-6 * np.abs(auto).max() and auto[0, p, k] != 0
  got = feats.grad.cpu().numpy().astype(np.float64)
  assert np.abs(got - auto).max() <= 1e-4 * np.abs(auto).max()
  assert abs(got[0, p, k] - fd) <= 1e-4 * np.abs(auto).max()


def test_net_feature_grad_on_a_real_net(small_net):
  from epos_amd import heads_train, loss, model, synthetic
  net, ckpt, mo, c, gt = small_net
  B, h, w, O, F = NET_B, net.out_h, net.out_w, NET_O, NET_F
  K = int(net.decoder_out.shape[-1])
  values, bad, dX = heads_train.net_feature_grad(net, gt, ckpt, WEIGHTS, 'pooled')
  assert values.shape == (4,) and values.dtype == torch.float64 and bad.tolist() == [0] * B
  assert dX.dtype == torch.float32 and tuple(dX.shape) == (B * h * w, K)
  # the same as the three calls by hand
  logits = net_logits(net)
  sums, counts, _ = loss.loss_terms(logits, gt)
  values2, scales = loss.loss_values(sums, counts, WEIGHTS, 'pooled')
  assert torch.equal(values, values2)
  hand = heads_train.heads_input_grad(logits, gt, scales, ckpt)
  assert torch.equal(dX, hand) and dX.abs().max() > 0
  # relu=True: zero where decoder_out is, the same elsewhere
  _, _, masked = heads_train.net_feature_grad(net, gt, ckpt, WEIGHTS, 'pooled', relu=True)
  keep = (net.decoder_out > 0).reshape(-1, K)
  assert keep.any() and (~keep).any()
  assert torch.equal(masked[keep], dX[keep]) and not masked[~keep].view(torch.int32).any()
  assert torch.equal(masked, heads_train.heads_input_grad(logits, gt, scales, ckpt,
                                                          relu_of=net.decoder_out))
  # against the helper on the device's own logit gradients
  d = [t.cpu().numpy() for t in loss.loss_grads(logits, gt, scales)]
  cls, frag = heads_wgrad_ref.classes(c, IGNORE)
  Ws = [ckpt[heads_train.variable_names(k)[0]] for k in KEYS]
  sums_r, abs_r, n_active = ref.dgrad(*d, *Ws, cls, frag)
  ok, worst = ref.within(dX.cpu().numpy(), sums_r, abs_r, n_active)
  assert ok, worst
  # a bf16 net is refused
  net16 = model.get_net(ckpt, 1, NET_H, NET_W, O, F, mo, 'cuda:0', precision='bf16')
  net16.forward_logits(synthetic.image(0, NET_H, NET_W)[None].astype(np.float32))
  gt1 = {k: v[:1] for k, v in gt.items()}
  with pytest.raises(TypeError, match='bf16 decoder_out is not supported'):
    heads_train.net_feature_grad(net16, gt1, ckpt)
