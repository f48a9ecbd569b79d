"""Host side of the backward pass through ASPP: the numpy restatements
(tests/helpers/aspp_grad_ref.py) and the chain of trainer.aspp_grads in numpy against torch's fp64
autograd through a torch.nn ASPP, the binding of the new symbols, both entries' host-side
refusals, weights.aspp_layers, what a dry-run plan records, and the wrapper's cut of K."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import aspp_grad_ref as aref                           # noqa: E402
from tests.helpers import decoder_backward_ref as ref                     # noqa: E402
from tests.helpers import pointwise_wgrad_ref as wref                     # noqa: E402

INVALID = -1                                  # EPOS_E_INVALID
EPS = 1e-5


# ------------------------------------------------------------- autograd ---
def test_the_chain_in_numpy_agrees_with_torch_fp64_autograd():
  """pre -> ReLU -> five branches (a global mean -> 1x1 -> broadcast; a 1x1; two separable convs
  at rates 1 and 2) -> concat -> 1x1 projection, frozen batch norms throughout, with a random
  cotangent at the projection's pre-activation: every branch's weight and batch-norm gradients
  and the gradient at `pre`, chained as trainer.aspp_grads chains the kernels, to 1e-12."""
  B, H, Wd, C, N, rates = 2, 7, 9, 8, 4, (1, 2)
  P, M = H * Wd, B * H * Wd
  rng = np.random.RandomState(7)
  f64 = np.float64

  def bn_of(n):
    gamma = (0.5 + rng.rand(n)) * np.where(np.arange(n) % 3 == 0, -1, 1)
    b = dict(gamma=gamma, beta=0.3 * rng.randn(n), mean=0.2 * rng.randn(n),
             var=0.2 + rng.rand(n))
    return {k: v.astype(np.float32).astype(f64) for k, v in b.items()}   # fp32 values, as stored
  pw_scopes = ['image_pooling', 'aspp0'] + ['aspp%d_pointwise' % i for i in (1, 2)]
  dw_scopes = ['aspp%d_depthwise' % i for i in (1, 2)]
  Wm = {s: 0.5 * rng.randn(C, N) for s in pw_scopes}
  Wm.update({s: 0.5 * rng.randn(3, 3, C, 1) for s in dw_scopes})
  bn = {s: bn_of(N) for s in pw_scopes}
  bn.update({s: bn_of(C) for s in dw_scopes})
  Wc, bnc = 0.5 * rng.randn(N * 4, N), bn_of(N)
  pre = rng.randn(B, H, Wd, C)
  G = rng.randn(M, N)                                      # the cotangent: d_proj

  leaves = {}

  def leaf(name, a):
    leaves[name] = torch.from_numpy(np.asarray(a, f64)).requires_grad_()
    return leaves[name]

  def bn_pre(z, s):
    b = bn[s]
    rstd = 1.0 / torch.sqrt(torch.from_numpy(b['var']) + EPS)
    g, be = leaf(s + '/gamma', b['gamma']), leaf(s + '/beta', b['beta'])
    return (z - torch.from_numpy(b['mean'])) * (g * rstd) + be
  pre_t = leaf('pre', pre)
  x = torch.relu(pre_t)
  pooled = x.mean(dim=(1, 2))
  pf = torch.relu(bn_pre(pooled @ leaf('image_pooling/w', Wm['image_pooling']), 'image_pooling'))
  parts = [pf[:, None, None, :].expand(B, H, Wd, N)]
  parts.append(torch.relu(bn_pre(x @ leaf('aspp0/w', Wm['aspp0']), 'aspp0')))
  acts = {}
  for i, r in enumerate(rates, 1):
    dws, pws = 'aspp%d_depthwise' % i, 'aspp%d_pointwise' % i
    wt = leaf(dws + '/w', Wm[dws])
    conv = torch.nn.functional.conv2d(
        x.permute(0, 3, 1, 2), wt[:, :, :, 0].permute(2, 0, 1).unsqueeze(1), padding=r,
        dilation=r, groups=C).permute(0, 2, 3, 1)
    a = torch.relu(bn_pre(conv, dws))
    acts[i] = a.detach().numpy()
    parts.append(torch.relu(bn_pre(a @ leaf(pws + '/w', Wm[pws]), pws)))
  cat = torch.cat(parts, dim=-1)
  sc_c = bnc['gamma'] / np.sqrt(bnc['var'] + EPS)
  z = cat.reshape(M, -1) @ torch.from_numpy(Wc * sc_c[None, :])
  (z * torch.from_numpy(G)).sum().backward()

  # the chain in numpy, with the restatements
  def scale_of(s):
    return bn[s]['gamma'] / np.sqrt(bn[s]['var'] + EPS)

  def wgrads(A, Gs, s, w):
    S, g, _, _ = wref.sums(A, Gs)
    b = bn[s]
    return wref.close(S, g, w, b['gamma'], b['mean'], b['var'], EPS, scale=scale_of(s))
  got = {}
  xh, cath = x.detach().numpy(), cat.detach().numpy()
  D_cat, _ = ref.pointwise_dgrad(G, Wc * sc_c[None, :], mask=cath.reshape(M, -1))
  D_cat = D_cat.reshape(B, H, Wd, -1)
  branch = lambda s: D_cat[..., N * s:N * (s + 1)]           # noqa: E731
  g_pool, _ = aref.pool_broadcast_ref(branch(0).reshape(B, P, N))
  pooledh = pooled.detach().numpy()
  got['image_pooling'] = wgrads(pooledh, g_pool, 'image_pooling', Wm['image_pooling'])
  d_pooled, _ = ref.pointwise_dgrad(g_pool, Wm['image_pooling'] * scale_of('image_pooling'))
  got['aspp0'] = wgrads(xh.reshape(M, C), branch(1).reshape(M, N), 'aspp0', Wm['aspp0'])
  E0, _ = ref.pointwise_dgrad(branch(1).reshape(M, N), Wm['aspp0'] * scale_of('aspp0'))
  terms = []
  for i, r in enumerate(rates, 1):
    dws, pws = 'aspp%d_depthwise' % i, 'aspp%d_pointwise' % i
    A = acts[i].reshape(M, C)
    got[pws] = wgrads(A, branch(i + 1).reshape(M, N), pws, Wm[pws])
    D, _ = ref.pointwise_dgrad(branch(i + 1).reshape(M, N), Wm[pws] * scale_of(pws), mask=A)
    D4 = D.reshape(B, H, Wd, C)
    T, t, _, _ = ref.depthwise_wgrad(xh, D4, r)
    b = bn[dws]
    got[dws] = wref.close(T, t, Wm[dws].reshape(9, C), b['gamma'], b['mean'], b['var'], EPS,
                          scale=scale_of(dws))
    terms.append((D4, Wm[dws].reshape(9, C) * scale_of(dws)[None, :], r))
  d_enc = aref.aspp_join_ref((B, H, Wd, C), depthwise=terms, plain=[E0], pooled=(d_pooled, P),
                             Y=xh, dtype=np.float64)

  def close_to(g, want, what):
    err = np.abs(g - want).max()
    assert np.abs(want).max() > 0 and err <= 1e-12 * np.abs(want).max(), (what, err)
  for s in pw_scopes + dw_scopes:
    dW, dgamma, dbeta = got[s]
    close_to(dW.reshape(leaves[s + '/w'].shape), leaves[s + '/w'].grad.numpy(), s + ' dW')
    close_to(dgamma, leaves[s + '/gamma'].grad.numpy(), s + ' dgamma')
    close_to(dbeta, leaves[s + '/beta'].grad.numpy(), s + ' dbeta')
  close_to(d_enc, pre_t.grad.numpy(), 'd_enc')
  assert (pre <= 0).any() and not d_enc[pre <= 0].any()
  # the bit-exact restatement is that same sum on fp32 inputs, rounded once
  t32 = [(D.astype(np.float32), w.astype(np.float32), r) for D, w, r in terms]
  E32, p32, x32 = E0.astype(np.float32), d_pooled.astype(np.float32), xh.astype(np.float32)
  exact = aref.aspp_join_ref((B, H, Wd, C), [(D.astype(f64), w.astype(f64), r)
                                             for D, w, r in t32], [E32.astype(f64)],
                             (p32.astype(f64), P), dtype=np.float64)
  bits = aref.aspp_join_ref((B, H, Wd, C), t32, [E32], (p32, P))
  assert bits.dtype == np.float32 and np.array_equal(bits, exact.astype(np.float32))
  masked = aref.aspp_join_ref((B, H, Wd, C), t32, [E32], (p32, P), Y=x32)
  assert np.array_equal(masked, np.where(x32 <= 0, np.float32(0), bits))
  assert not masked[x32 <= 0].view(np.uint32).any()
  # one depthwise term alone is the depthwise input gradient's restatement
  D, w, r = t32[1]
  assert np.array_equal(aref.aspp_join_ref((B, H, Wd, C), [(D, w, r)], Y=x32).view(np.uint32),
                        ref.depthwise_dgrad(D, w, r, Y=x32).view(np.uint32))


def test_the_restatements_on_small_cases():
  # a tap outside the image adds +0.0, never 0 * inf
  D = np.full((1, 2, 2, 4), np.inf, np.float32)
  D[0, 0, 0] = 1.0
  w = np.zeros((9, 4), np.float32)
  w[4] = 2.0
  out = aref.aspp_join_ref((1, 2, 2, 4), [(D, w, 2)])
  assert out[0, 0, 0].tolist() == [2.0] * 4 and np.isinf(out[0, 1, 1]).all()
  # plain terms, the division and the mask: -0.0 masks, a NaN does not
  E = np.float32([[[[1.0, -2.0, 3.0, 4.0]]]])
  pool = np.float32([[3.0, 3.0, 3.0, 3.0]])
  Y = np.float32([[[[1.0, -0.0, np.nan, 0.0]]]])
  out = aref.aspp_join_ref((1, 1, 1, 4), plain=[E, E], pooled=(pool, 3), Y=Y)
  assert out.tolist() == [[[[3.0, 0.0, 7.0, 0.0]]]] and not out.view(np.uint32)[0, 0, 0, 1]
  third = aref.aspp_join_ref((1, 1, 1, 4), pooled=(np.float32([[1, 1, 1, 1]]), 3))
  assert third[0, 0, 0, 0] == np.float32(1.0 / 3.0)
  # the broadcast's adjoint: the exact sum where a running fp32 (or fp64) sum loses the ones
  Dp = np.zeros((1, 5, 4), np.float32)
  Dp[0, :, 0] = [1e30, 1.0, -1e30, 1.0, 1.0]
  Dp[0, :, 1] = [1, 2, 3, 4, 5]
  s, b = aref.pool_broadcast_ref(Dp)
  assert s[0].tolist() == [3.0, 15.0, 0.0, 0.0]
  assert b[0, 1] == 2.0 ** -24 * 15 + 21 * 2.0 ** -52 * 15 and b[0, 2] == 0


# -------------------------------------------------------------- binding ---
C_NAMES = {ctypes.c_int: 'int', ctypes.c_int64: 'int64_t', ctypes.c_float: 'float',
           ctypes.c_double: 'double'}


def test_symbols_are_declared_bound_and_exported():
  from epos_amd import _lib
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  assert '/* ASPP gradients (csrc/aspp_grad.hip' in header
  assert 'g[b,c] = fl32( sum_p (double)D[b P + p, c] )' in header
  assert '(double)Pool[b, c] / (double)pool_div' in header
  assert '#define EPOS_ABI_VERSION 7' in header
  header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  for name, ctype, n_args in (('epos_pool_broadcast_dgrad_range_pixels', 'int64_t', 3),
                              ('epos_pool_broadcast_dgrad_workspace_bytes', 'int64_t', 3),
                              ('epos_pool_broadcast_dgrad_f32', 'int', 9),
                              ('epos_aspp_join_dgrad_f32', 'int', 2)):
    restype, argtypes = _lib.SYMBOLS[name]
    assert C_NAMES[restype] == ctype
    decl = re.search(r'\b%s %s\s*\(([^)]*)\)\s*;' % (ctype, name), header)
    assert decl, name
    args = [a.strip() for a in decl.group(1).split(',')]
    assert len(args) == len(argtypes) == n_args, name
    for arg, t in zip(args, argtypes):                     # pointer or the scalar type by name
      if '*' in arg:
        assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), arg
      else:
        assert arg.split()[0] == C_NAMES[t], arg
    assert getattr(ctypes.CDLL(_lib.lib_path()), name)     # exported by the built library
  assert ctypes.sizeof(_lib.AsppJoinDw) == 32 and ctypes.sizeof(_lib.AsppJoinPlain) == 16
  assert ctypes.sizeof(_lib.AsppJoinArgs) == 248
  body = re.search(r'typedef struct EposAsppJoinArgs \{(.*?)\} EposAsppJoinArgs;', header,
                   flags=re.S).group(1)
  names = re.findall(r'(\w+)(?:\[\d\])?\s*[;,]', body)
  assert names == [f[0] for f in _lib.AsppJoinArgs._fields_]
  for const, key in (('PIXEL', 'pixel'), ('SLICE32', 'slice32'), ('SLICE64', 'slice64'),
                     ('SLICE32X2', 'slice32x2'), ('SLICE32X4', 'slice32x4')):
    value = int(re.search(r'#define EPOS_ASPP_JOIN_%s (\d)' % const, header).group(1))
    assert _lib.ASPP_JOIN_PARTITIONS[key] == value
  assert _lib.ASPP_JOIN_PARTITIONS['shipped'] == 0
  assert os.path.exists(os.path.join(ROOT, 'epos_amd', 'csrc', 'aspp_grad.hip'))
  assert _lib.load().epos_abi_version() == 7               # added without a version change


def test_pool_broadcast_host_side_refusals():
  from epos_amd import _lib
  lib = _lib.load()
  fake = 4096

  def call(**over):
    f = dict(D=fake, ldd=8, g=fake * 2, ldg=8, B=2, P=10, C=8, workspace=fake * 3)
    f.update(over)
    return lib.epos_pool_broadcast_dgrad_f32(f['D'], f['ldd'], f['g'], f['ldg'], f['B'], f['P'],
                                             f['C'], f['workspace'], None)
  positive = b'B, P and C must be positive'
  for over, msg in ((dict(B=0), positive), (dict(P=0), positive), (dict(C=-4), positive),
                    (dict(C=6), b'C must be a multiple of 4'),
                    (dict(B=65536), b'too many pixels'), (dict(P=(1 << 40) + 1), b'too many pixels'),
                    (dict(ldd=4), b'ldd must be >= C and a multiple of 4'),
                    (dict(ldd=10), b'ldd must be >= C and a multiple of 4'),
                    (dict(ldg=7), b'ldg must be >= C and a multiple of 4'),
                    (dict(D=None), b'null pointer'), (dict(g=None), b'null pointer'),
                    (dict(D=fake + 4), b'D and g must be 16-byte aligned'),
                    (dict(g=fake * 2 + 8), b'D and g must be 16-byte aligned'),
                    (dict(g=fake), b'g may not start at D'),
                    (dict(P=65, workspace=None), b'the workspace must be given, 8-byte aligned'),
                    (dict(P=65, workspace=fake * 3 + 4),
                     b'the workspace must be given, 8-byte aligned')):
    assert call(**over) == INVALID, over
    assert lib.epos_last_error() == b'epos_pool_broadcast_dgrad_f32: ' + msg, over
  # the cut into ranges is a function of P alone
  pixels, nbytes = (lib.epos_pool_broadcast_dgrad_range_pixels,
                    lib.epos_pool_broadcast_dgrad_workspace_bytes)
  assert pixels(1, 1, 4) == pixels(8, 64, 2048) == 64 and nbytes(3, 64, 12) == 0
  assert nbytes(2, 65, 12) == 8 * 2 * 2 * 12 and nbytes(2, 192, 256) == 8 * 3 * 2 * 256
  assert pixels(1, 4800, 256) == pixels(8, 4800, 8) == 75 and nbytes(1, 4800, 256) == 8 * 64 * 256
  assert pixels(0, 4, 4) == INVALID and nbytes(1, 4, 6) == INVALID


def test_aspp_join_host_side_refusals():
  from epos_amd import _lib
  lib = _lib.load()
  fake = 4096

  def call(dw=None, plain=None, **over):
    f = dict(B=1, H=4, W=4, C=8, n_dw=2, n_plain=1, Pool=fake * 10, ldp=8, pool_div=16,
             Y=fake * 11, ldy=8, dX=fake * 12, ldx=8, partition=0)
    f.update(over)
    a = _lib.AsppJoinArgs(**f)
    for t in range(4):
      d = dict(D=fake * (1 + t), ldd=8, w9c=fake * (5 + t), rate=1 + t)
      d.update((dw or {}).get(t, {}))
      a.dw[t] = _lib.AsppJoinDw(**d)
    for j in range(2):
      e = dict(E=fake * (13 + j), lde=8)
      e.update((plain or {}).get(j, {}))
      a.plain[j] = _lib.AsppJoinPlain(**e)
    return lib.epos_aspp_join_dgrad_f32(ctypes.byref(a), None)
  positive = b'B, H, W and C must be positive'
  aligned = b'every pointer must be 16-byte aligned'
  starts = b'dX may not start at an input'
  for kw, msg in (
      (dict(B=0), positive), (dict(W=-1), positive), (dict(C=0), positive),
      (dict(C=6), b'C must be a multiple of 4'), (dict(H=(1 << 30) + 1), b'too many pixels'),
      (dict(n_dw=5), b'n_dw must be in 0..4'), (dict(n_dw=-1), b'n_dw must be in 0..4'),
      (dict(n_plain=3), b'n_plain must be in 0..2'),
      (dict(n_dw=0, n_plain=0, Pool=None), b'at least one term must be present'),
      (dict(dX=None), b'null pointer'), (dict(dw={1: dict(D=None)}), b'null pointer'),
      (dict(dw={0: dict(w9c=None)}), b'null pointer'), (dict(plain={0: dict(E=None)}),
                                                        b'null pointer'),
      (dict(dw={0: dict(rate=0)}), b'rate must be >= 1'),
      (dict(dw={1: dict(rate=(1 << 20) + 1)}), b'rate must be >= 1'),
      (dict(dw={1: dict(ldd=4)}), b'ldd must be >= C and a multiple of 4'),
      (dict(dw={0: dict(ldd=10)}), b'ldd must be >= C and a multiple of 4'),
      (dict(plain={0: dict(lde=9)}), b'lde must be >= C and a multiple of 4'),
      (dict(ldp=6), b'ldp must be >= C and a multiple of 4'),
      (dict(ldy=4), b'ldy must be >= C and a multiple of 4'),
      (dict(ldx=7), b'ldx must be >= C and a multiple of 4'),
      (dict(pool_div=0), b'pool_div must be >= 1'),
      (dict(dX=fake * 12 + 4), aligned), (dict(dw={1: dict(D=fake * 2 + 8)}), aligned),
      (dict(dw={0: dict(w9c=fake * 5 + 4)}), aligned), (dict(plain={0: dict(E=fake * 13 + 4)}),
                                                        aligned),
      (dict(Pool=fake * 10 + 8), aligned), (dict(Y=fake * 11 + 4), aligned),
      (dict(dX=fake * 2), starts), (dict(dX=fake * 13), starts), (dict(dX=fake * 10), starts),
      (dict(dX=fake * 11), starts),
      (dict(partition=6), b'unknown partition'), (dict(partition=-1), b'unknown partition')):
    assert call(**kw) == INVALID, kw
    assert lib.epos_last_error() == b'epos_aspp_join_dgrad_f32: ' + msg, kw
  # what n_dw and n_plain do not count is not looked at
  assert call(dw={2: dict(D=None, rate=0)}, plain={1: dict(E=None)}, B=0) == INVALID
  assert lib.epos_aspp_join_dgrad_f32(None, None) == INVALID
  assert lib.epos_last_error() == b'epos_aspp_join_dgrad_f32: null args'


# ---------------------------------------------------------- the package ---
def test_aspp_layers_and_the_pinned_tables():
  from epos_amd import net, weights as W
  pw, dw = W.aspp_layers((12, 24, 36))
  assert list(pw) == ['image_pooling', 'aspp0', 'aspp1_pointwise', 'aspp2_pointwise',
                      'aspp3_pointwise']
  assert list(dw) == ['aspp1_depthwise', 'aspp2_depthwise', 'aspp3_depthwise']
  assert set(pw.values()) | set(dw.values()) == {net.HEAD_BN_EPS} == {1e-5}
  pw, dw = W.aspp_layers(())
  assert list(pw) == ['image_pooling', 'aspp0'] and dw == {}
  assert W.POINTWISE_CHAIN_LAYERS == {'decoder/decoder_conv0_pointwise': 1e-5,
                                      'decoder/feature_projection0': 1e-5,
                                      'concat_projection': 1e-5}
  assert W.DEPTHWISE_CHAIN_LAYERS == {'decoder/decoder_conv0_depthwise': 1e-5}
  assert W.DEPTHWISE_BACKWARD_LAYERS == {'decoder/decoder_conv1_depthwise': 1e-5}
  assert list(W.TRAINABLE_LAYERS) == ['logits/pred_obj_conf', 'logits/pred_frag_conf',
                                      'logits/pred_frag_loc', 'decoder/decoder_conv1_pointwise']
  assert len(W.trainable_variables()) == 9


@pytest.mark.parametrize('rates', [(12, 24, 36), ()])
def test_a_dry_run_records_every_aspp_operand(rates, monkeypatch):
  from epos_amd import net, trainer, weights as W
  from epos_amd._lib import EposError
  ckpt = W.random_init('xception_65', num_objs=2, num_frags=4, seed=0, atrous_rates=rates)
  plan = net.EposNet(ckpt, 2, 64, 64, 2, 4, dry_run=True, atrous_rates=rates)
  ap = plan.aspp_operands()
  assert sorted(ap) == sorted(['encoder', 'encoder_relu', 'pooled', 'pool_feat', 'aspp_concat',
                               'rates', 'pointwise', 'depthwise'])
  enc = ap['encoder']
  assert tuple(enc.shape) == (2, 8, 8, 2048) and enc.data_ptr() == plan.encoder.data_ptr()
  assert ap['encoder_relu'] is True and ap['rates'] == rates
  assert tuple(ap['pooled'].shape) == (2, 2048) and tuple(ap['pool_feat'].shape) == (2, 256)
  assert ap['aspp_concat'] is plan.aspp_concat
  assert tuple(ap['aspp_concat'].shape) == (2, 8, 8, 256 * (2 + len(rates)))
  pw, dw = W.aspp_layers(rates)
  assert list(ap['pointwise']) == list(pw) and list(ap['depthwise']) == list(dw)
  ip = ap['pointwise']['image_pooling']
  assert ip['a'] is ap['pooled'] and (ip['m'], ip['k'], ip['n'], ip['lda']) == (2, 2048, 256, 2048)
  assert not ip['presplit'] and ip['a_h2'] is None and ip['packs'] is None and ip['eps'] == 1e-5
  a0 = ap['pointwise']['aspp0']
  assert a0['a'] is plan.encoder and (a0['m'], a0['k'], a0['n']) == (128, 2048, 256)
  assert not a0['presplit']
  assert plan._expr_of(ap['pool_feat']) == 'relu(L:image_pooling)'
  for i, r in enumerate(rates, 1):
    d = ap['depthwise']['aspp%d_depthwise' % i]
    assert sorted(d) == sorted(['x', 'ldx', 'b', 'h', 'w', 'c', 'rate', 'w9c', 'bias', 'eps'])
    assert d['x'] is plan.encoder and d['rate'] == r and d['eps'] == 1e-5
    assert (d['b'], d['h'], d['w'], d['c'], d['ldx']) == (2, 8, 8, 2048, 2048)
    assert tuple(d['w9c'].shape) == (9, 2048)
    p = ap['pointwise']['aspp%d_pointwise' % i]
    assert plan._expr_of(p['a'], 0, 2048) == 'relu(L:aspp%d_depthwise)' % i
    assert (p['m'], p['k'], p['n']) == (128, 2048, 256) and p['presplit']
    assert plan._expr_of(plan.aspp_concat, 256 * (i + 1), 256) == 'relu(L:aspp%d_pointwise)' % i
  # the existing accessors keep refusing these names
  with pytest.raises(ValueError, match='aspp0'):
    plan.crossed_pointwise_operand('aspp0')
  with pytest.raises(ValueError, match='image_pooling'):
    plan.pointwise_constants('image_pooling')
  with pytest.raises(ValueError, match='aspp1_depthwise'):
    plan.crossed_depthwise_operand('aspp1_depthwise')
  with pytest.raises(ValueError, match='not an ASPP layer'):
    plan.aspp_constants('concat_projection')
  consts = plan.aspp_constants('aspp0')
  assert [tuple(t.shape) for t in consts] == [(1, 1, 2048, 256), (256,), (256,), (256,)]
  assert all(a is b for a, b in zip(consts, plan.aspp_constants('aspp0')))
  if rates:
    consts = plan.aspp_constants('aspp2_depthwise')
    assert [tuple(t.shape) for t in consts] == [(3, 3, 2048, 1), (2048,), (2048,), (2048,)]
  with pytest.raises(EposError, match='no CPU fallback'):                 # a dry run has no device
    trainer.aspp_grads(plan, None, {})
  bf16 = net.EposNet(ckpt, 2, 64, 64, 2, 4, dry_run=True, precision='bf16', atrous_rates=rates)
  with pytest.raises(NotImplementedError, match='bf16'):
    bf16.aspp_operands()
  # with the records off the plan is the same list of ops
  monkeypatch.setattr(W, 'aspp_layers', lambda r: ({}, {}))
  bare = net.EposNet(ckpt, 2, 64, 64, 2, 4, dry_run=True, atrous_rates=rates)
  assert bare.aspp_operands()['pointwise'] == {} and bare.aspp_operands()['depthwise'] == {}
  assert [n for n, _ in bare.ops] == [n for n, _ in plan.ops]
  assert bare.op_kind == plan.op_kind and bare.op_flops == plan.op_flops
  assert bare.op_bytes == plan.op_bytes
  assert sorted(bare.mode.layer_operands) == sorted(set(plan.mode.layer_operands) - set(pw))


def test_the_wrappers_cut_of_k():
  from epos_amd import decoder_train as DT
  assert DT.k_blocks(1) == [(0, 1)] and DT.k_blocks(1024) == [(0, 1024)]
  assert DT.k_blocks(1025) == [(0, 1024), (1024, 1025)]
  assert DT.k_blocks(1280) == [(0, 1024), (1024, 1280)]
  assert DT.k_blocks(2048) == [(0, 1024), (1024, 2048)]
  assert DT.k_blocks(2052) == [(0, 1024), (1024, 2048), (2048, 2052)]
  for K in (1, 1024, 1025, 1280, 2048, 2052):
    blocks = DT.k_blocks(K)
    assert blocks[0][0] == 0 and blocks[-1][1] == K
    assert all(a[1] == b[0] for a, b in zip(blocks, blocks[1:]))
    assert all(0 < k1 - k0 <= 1024 and k0 % 4 == 0 for k0, k1 in blocks)
  assert DT.k_blocks(1280, 640) == [(0, 640), (640, 1280)]
  with pytest.raises(ValueError):
    DT.k_blocks(0)
  with pytest.raises(ValueError):
    DT.k_blocks(8, 6)
  z = torch.zeros
  from epos_amd._lib import EposError
  with pytest.raises(EposError, match='no CPU fallback'):
    DT.pool_broadcast_grad(z(1, 2, 2, 8))
  with pytest.raises(EposError, match='no CPU fallback'):
    DT.aspp_join_grad(plain=[z(1, 2, 2, 8)])
