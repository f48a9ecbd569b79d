"""Host side of the backward pass through the decoder: the numpy restatement of the resize adjoint
(tests/helpers/resize_grad_ref.py) against the forward it is the adjoint of and against torch's
fp64 autograd, the binding of the new symbol and its host-side refusals, the new layer tables and
what the plan records for them."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import glue_ref                                        # noqa: E402
from tests.helpers import resize_grad_ref as ref                          # noqa: E402

INVALID = -1                                  # EPOS_E_INVALID
SIZES = [(3, 5, 5, 9), (5, 7, 5, 7), (12, 16, 24, 32), (60, 80, 120, 160), (7, 9, 4, 3),
         (4, 6, 1, 1), (2, 2, 3, 3)]


def _data(shape, seed):
  return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def _adjoint64(D, hi, wi):
  acc, mag, count = ref.resize_dgrad(D, hi, wi, dtype=np.longdouble)
  return acc.astype(np.float64), mag.astype(np.float64), count


@pytest.mark.parametrize('hi,wi,ho,wo', SIZES)
def test_adjoint_identity_with_the_forwards_own_coordinates(hi, wi, ho, wo):
  """<resize(X), D> == <X, adjoint(D)> in fp64, the resize being the one the plan runs: the
  weights of glue_ref._resize_coords_f32."""
  X = _data((2, hi, wi, 4), 1).astype(np.float64)
  D = _data((2, ho, wo, 4), 2)
  Wy, Wx = ref.axis_matrix(hi, ho), ref.axis_matrix(wi, wo)
  fwd = np.einsum('oy,bywc,pw->bopc', Wy, X, Wx)
  # the matrix form IS the forward: the fp32 kernel's restatement lies within its rounding of it
  f32, (tl, tr, bl, br) = glue_ref.resize_f32(X.astype(np.float32), ho, wo)
  mag = np.abs(tl) + np.abs(tr) + np.abs(bl) + np.abs(br)
  assert np.all(np.abs(f32 - fwd) <= 8 * 2.0 ** -24 * mag)
  adj, _, _ = _adjoint64(D, hi, wi)
  lhs, rhs = float((fwd * D).sum()), float((X * adj).sum())
  scale = float((np.abs(fwd) * np.abs(D)).sum())
  assert abs(lhs - rhs) <= 1e-13 * scale and scale > 0
  # and the loop of the restatement is the transpose of that matrix
  want = np.einsum('oy,bopc,pw->bywc', Wy, D.astype(np.float64), Wx)
  assert np.all(np.abs(adj - want) <= 1e-13 * np.abs(want).max())


@pytest.mark.parametrize('ni,no', [(3, 5), (5, 9), (5, 5), (60, 120), (80, 160), (12, 24),
                                   (7, 4), (9, 3), (4, 1), (2, 3), (59, 119)])
def test_every_output_index_spreads_a_weight_of_one(ni, no):
  Wm = ref.axis_matrix(ni, no)
  assert np.array_equal(Wm.sum(axis=1), np.ones(no))       # exactly: (1 - l) + l in fp64
  assert np.all(Wm >= 0) and np.all((Wm != 0).sum(axis=1) <= 2)
  for taps in ref.axis_taps(ni, no):
    assert len({i for i, _ in taps}) == len(taps) and all(0 <= i < ni for i, _ in taps)


def _torch_adjoint(D, hi, wi):
  B, ho, wo, C = D.shape
  x = torch.zeros((B, C, hi, wi), dtype=torch.float64, requires_grad=True)
  y = torch.nn.functional.interpolate(x, size=(ho, wo), mode='bilinear', align_corners=True)
  y.backward(torch.from_numpy(D.astype(np.float64)).permute(0, 3, 1, 2))
  return x.grad.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize('hi,wi,ho,wo', [(3, 5, 5, 9), (5, 7, 5, 7), (5, 3, 9, 5)])
def test_agrees_with_torch_fp64_autograd_where_the_ratio_is_exact(hi, wi, ho, wo):
  """(in - 1) / (out - 1) is 1/2 or 1: exact in fp32, so the fp32 coordinates are torch's."""
  D = _data((2, ho, wo, 4), 3)
  adj, _, _ = _adjoint64(D, hi, wi)
  want = _torch_adjoint(D, hi, wi)
  assert np.abs(want).max() > 0
  assert np.all(np.abs(adj - want) <= 1e-12 * np.abs(want).max())
  bits = ref.resize_dgrad(D, hi, wi)
  assert np.all(np.abs(bits - want) <= 2.0 ** -23 * np.abs(want) + 1e-12)


@pytest.mark.parametrize('hi,wi,ho,wo', [(60, 80, 120, 160), (12, 16, 24, 32), (7, 15, 75, 47)])
def test_agrees_with_torch_fp64_autograd_within_the_coordinate_error(hi, wi, ho, wo):
  """Where the ratio is not exact in fp32 the coordinates differ from torch's by at most
  d = 4 * 2^-24 * max(hi, wi) (glue_ref.resize_bound), so each weight wy wx by at most 2 d, a
  sample that fp32 moved into the neighbouring cell included (there a weight below d sits on
  another source): |adjoint - torch| <= 2 d sum |D| over the union of both footprints."""
  D = _data((1, ho, wo, 4), 4)
  adj, _, _ = _adjoint64(D, hi, wi)
  want = _torch_adjoint(D, hi, wi)
  d = 4 * 2.0 ** -24 * max(hi, wi)
  Fy = ((ref.axis_matrix(hi, ho) != 0) | (ref.axis_matrix(hi, ho, exact=True) != 0)) * 1.0
  Fx = ((ref.axis_matrix(wi, wo) != 0) | (ref.axis_matrix(wi, wo, exact=True) != 0)) * 1.0
  near = np.einsum('oy,bopc,pw->bywc', Fy, np.abs(D).astype(np.float64), Fx)
  err = np.abs(adj - want)
  print('%dx%d -> %dx%d: max |adjoint - torch| / bound = %.3g' % (
      hi, wi, ho, wo, float((err / (2 * d * near + 1e-300)).max())))
  assert np.all(err <= 2 * d * near + 1e-13 * np.abs(want).max())
  assert err.max() > 0                        # the coordinates do differ: the case is not vacuous


def _moved(ni, no):
  f32, _, _ = glue_ref._resize_coords_f32(ni, no)
  exact, _, _ = glue_ref._resize_coords_exact(ni, no)
  return np.nonzero(f32 != exact)[0], f32, exact


@pytest.mark.parametrize('ni,no,where', [(7, 75, [37, 74]), (15, 47, [23, 46]), (8, 24, [23])])
def test_fp32_moves_a_sample_into_the_neighbouring_cell(ni, no, where):
  """Sizes at which fp32 rounding puts an output index into another cell than exact arithmetic
  does: o s rounds to just below an integer that o (in - 1) / (out - 1) is exactly -- at the last
  index, and at 7 -> 75 and 15 -> 47 in the interior too. The adjoint follows the forward there,
  not the exact positions: a closed form of (i +- 1) / s would name other sources."""
  moved, f32, exact = _moved(ni, no)
  assert moved.tolist() == where
  for o in moved:
    taps = ref.axis_taps(ni, no)[int(o)]
    assert taps[0][0] == int(f32[o]) == int(exact[o]) - 1 and len(taps) == 2
    assert taps[1][0] == int(exact[o]) and 1.0 - taps[1][1] <= 2.0 ** -20   # nearly all of it
  assert not np.array_equal(ref.axis_matrix(ni, no) != 0, ref.axis_matrix(ni, no, exact=True) != 0)


def test_no_sample_moves_at_the_workloads_sizes():
  """60 -> 120 and 80 -> 160 (59 / 119, 79 / 159), and the small net's 12 -> 24 and 16 -> 32: the
  fp32 coordinates differ from the exact ones (by up to 4e-6) but every index stays in its
  cell -- o s hits in - 1 exactly at the last index. (A moved sample was expected at 60 -> 120
  when the adjoint was designed; there is none, so the moved samples are tested at the sizes
  above, on the device too.)"""
  for ni, no in ((60, 120), (80, 160), (12, 24), (16, 32)):
    moved, _, _ = _moved(ni, no)
    assert moved.size == 0, (ni, no)
    _, _, l32 = glue_ref._resize_coords_f32(ni, no)
    _, _, le = glue_ref._resize_coords_exact(ni, no)
    assert 0 < np.abs(l32.astype(np.float64) - le).max() <= 4 * 2.0 ** -24 * ni


def test_restatement_is_within_its_bound_and_masks():
  hi, wi, ho, wo = 5, 6, 11, 13
  D = _data((2, ho, wo, 4), 5)
  Y = _data((2, hi, wi, 4), 6)
  Y[0, 0, 0, 0], Y[0, 0, 0, 1], Y[0, 0, 0, 2] = -0.0, np.nan, 0.0
  exact, mag, count = ref.resize_dgrad(D, hi, wi, dtype=np.longdouble)
  got = ref.resize_dgrad(D, hi, wi)
  assert np.all(np.abs(got.astype(np.float64) - exact.astype(np.float64)) <=
                ref.bound(exact, mag, count))
  assert count.min() == 9 and count.max() == 25      # 5 -> 11, 6 -> 13: up to 5 x 5
  masked = ref.resize_dgrad(D, hi, wi, Y=Y)
  off = Y <= 0
  assert off[0, 0, 0, 0] and not off[0, 0, 0, 1] and off[0, 0, 0, 2]
  assert np.array_equal(masked.view(np.uint32)[off], np.zeros(int(off.sum()), np.uint32))
  assert np.array_equal(masked.view(np.uint32)[~off], got.view(np.uint32)[~off])
  # the identity yields the bytes of D
  same = ref.resize_dgrad(D, ho, wo)
  assert np.array_equal(same.view(np.uint32), D.view(np.uint32))


# ------------------------------------------------------------- the C ABI ---
def test_symbol_is_declared_bound_and_exported():
  from epos_amd import _lib
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  assert '/* Resize input gradient (csrc/resize_grad.hip' in header
  section = header[header.index('/* Resize input gradient ('):header.index('/* Weight update (')]
  for phrase in ('rows ascending, columns ascending within a row', 'never by a closed form',
                 '(n + 16) 2^-52 sum |w||D|', 'the image-pooling broadcast'):
    assert phrase in section, phrase
  assert '#define EPOS_ABI_VERSION 7' in header
  bare = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  restype, argtypes = _lib.SYMBOLS['epos_resize_bilinear_dgrad_f32']
  decl = re.search(r'\bint epos_resize_bilinear_dgrad_f32\s*\(([^)]*)\)\s*;', bare)
  assert decl and restype is ctypes.c_int
  args = [a.strip() for a in decl.group(1).split(',')]
  assert len(args) == len(argtypes) == 13
  for arg, t in zip(args, argtypes):
    if '*' in arg:
      assert t is ctypes.c_void_p, arg
    else:
      assert {'int': ctypes.c_int, 'int64_t': ctypes.c_int64}[arg.split()[0]] is t, arg
  assert getattr(ctypes.CDLL(_lib.lib_path()), 'epos_resize_bilinear_dgrad_f32')
  assert os.path.exists(os.path.join(ROOT, 'epos_amd', 'csrc', 'resize_grad.hip'))
  assert _lib.load().epos_abi_version() == 7               # added without a version change


def test_host_side_refusals():
  from epos_amd import _lib
  lib = _lib.load()
  fake = 4096

  def call(**over):
    f = dict(D=fake, ldd=8, Y=fake * 2, ldy=8, dX=fake * 3, ldx=8, B=1, Hi=3, Wi=4, Ho=5, Wo=7,
             C=8)
    f.update(over)
    return lib.epos_resize_bilinear_dgrad_f32(f['D'], f['ldd'], f['Y'], f['ldy'], f['dX'],
                                              f['ldx'], f['B'], f['Hi'], f['Wi'], f['Ho'], f['Wo'],
                                              f['C'], None)
  positive = b'B, Hi, Wi, Ho, Wo and C must be positive'
  broadcast = b'a source of one row or column broadcasts: its adjoint is a sum, not this entry'
  aligned = b'D, Y and dX must be 16-byte aligned'
  for over, msg in ((dict(B=0), positive), (dict(Hi=0), positive), (dict(Wi=-1), positive),
                    (dict(Ho=0), positive), (dict(Wo=0), positive), (dict(C=0), positive),
                    (dict(C=6), b'C must be a multiple of 4'),
                    (dict(Hi=1 << 23), b'too many pixels'),
                    (dict(Hi=1), broadcast), (dict(Wi=1), broadcast),
                    (dict(Hi=1, Wi=1, Ho=1), broadcast),
                    (dict(ldd=4), b'ldd must be >= C and a multiple of 4'),
                    (dict(ldd=10), b'ldd must be >= C and a multiple of 4'),
                    (dict(ldx=6), b'ldx must be >= C and a multiple of 4'),
                    (dict(ldy=9), b'ldy must be >= C and a multiple of 4'),
                    (dict(D=None), b'null pointer'), (dict(dX=None), b'null pointer'),
                    (dict(D=fake + 4), aligned), (dict(Y=fake * 2 + 8), aligned),
                    (dict(dX=fake * 3 + 4), aligned),
                    (dict(dX=fake), b'dX may not start at D'),
                    (dict(dX=fake * 2), b'dX may not start at Y')):
    assert call(**over) == INVALID, over
    assert lib.epos_last_error() == b'epos_resize_bilinear_dgrad_f32: ' + msg, over


def test_wrapper_needs_a_device():
  from epos_amd import decoder_train as DT
  from epos_amd import trainer
  from epos_amd._lib import EposError
  with pytest.raises(EposError, match='no CPU fallback'):
    DT.resize_input_grad(torch.zeros(1, 4, 4, 8), (2, 2))
  assert callable(trainer.decoder_grads)


# ------------------------------------------------------------- the tables ---
def test_the_new_tables():
  from epos_amd import net, weights as W
  assert list(W.POINTWISE_CHAIN_LAYERS) == [
      'decoder/decoder_conv0_pointwise', 'decoder/feature_projection0', 'concat_projection']
  assert list(W.DEPTHWISE_CHAIN_LAYERS) == ['decoder/decoder_conv0_depthwise']
  for table in (W.POINTWISE_CHAIN_LAYERS, W.DEPTHWISE_CHAIN_LAYERS):
    assert all(eps == net.HEAD_BN_EPS for eps in table.values())
    assert not set(table) & set(W.TRAINABLE_LAYERS)
    assert not set(table) & set(W.DEPTHWISE_BACKWARD_LAYERS)
  assert not set(W.POINTWISE_CHAIN_LAYERS) & set(W.DEPTHWISE_CHAIN_LAYERS)
  # nothing became trainable
  assert len(W.TRAINABLE_LAYERS) == 4 and len(W.trainable_variables()) == 9
  assert list(W.DEPTHWISE_BACKWARD_LAYERS) == [W.DECODER_CONV1_DEPTHWISE]
  specs = {s[1]: s for s in W.variable_specs('xception_65')}
  for scope in list(W.POINTWISE_CHAIN_LAYERS) + list(W.DEPTHWISE_CHAIN_LAYERS):
    assert scope in specs


def _op_list(plan):
  return ([name for name, _ in plan.ops], dict(plan.op_kind), dict(plan.op_flops),
          dict(plan.op_bytes), len(plan._keep))


@pytest.mark.parametrize('variant', ['xception_65', 'resnet_v1_50'])
def test_a_dry_run_records_the_operands_and_launches_nothing_more(variant, monkeypatch):
  from epos_amd import net, trainer, weights as W
  from epos_amd._lib import EposError
  ckpt = W.random_init(variant, num_objs=2, num_frags=4, seed=0)
  plan = net.EposNet(ckpt, 2, 64, 96, 2, 4, dry_run=True, model_variant=variant)
  ch = plan.chain_operands()
  eh, ew = ch['encoder_hw']
  assert ch['decoder_hw'] == ch['low_level_hw'] == (16, 24) and (eh, ew) == (8, 12)
  assert tuple(ch['decoder_concat'].shape) == (2, 16, 24, 304)
  assert tuple(ch['concat_projection'].shape) == (2, eh, ew, 256)
  assert tuple(ch['aspp_concat'].shape) == (2, eh, ew, 1280)
  assert tuple(ch['low_level'].shape) == (2, 16, 24, 256)
  assert ch['decoder_concat'].data_ptr() == plan.decoder_concat.data_ptr()
  assert ch['concat_projection'] is plan.concat_projection and ch['aspp_concat'] is plan.aspp_concat

  dw = plan.crossed_depthwise_operand()
  assert sorted(dw) == sorted(plan.depthwise_operand())
  assert (dw['b'], dw['h'], dw['w'], dw['c'], dw['rate']) == (2, 16, 24, 304, 1)
  assert dw['x'].data_ptr() == ch['decoder_concat'].data_ptr() and dw['ldx'] == 304
  assert tuple(dw['w9c'].shape) == (9, 304) and dw['eps'] == net.HEAD_BN_EPS
  consts = plan.crossed_depthwise_constants()
  assert [tuple(t.shape) for t in consts] == [(3, 3, 304, 1), (304,), (304,), (304,)]
  assert all(a is b for a, b in zip(consts, plan.crossed_depthwise_constants()))

  want = {W.DECODER_CONV0_POINTWISE: (2 * 16 * 24, 304, 256),
          W.FEATURE_PROJECTION0: (2 * 16 * 24, 256, 48),
          W.CONCAT_PROJECTION: (2 * eh * ew, 1280, 256)}
  for name, (m, k, n) in want.items():
    op = plan.crossed_pointwise_operand(name)
    assert sorted(op) == sorted(['a', 'lda', 'm', 'k', 'n', 'presplit', 'a_h2', 'packs', 'eps'])
    assert (op['m'], op['k'], op['n']) == (m, k, n), name
    assert op['packs'] is None and op['eps'] == W.POINTWISE_CHAIN_LAYERS[name]
    consts = plan.pointwise_constants(name)
    assert [tuple(t.shape) for t in consts] == [(1, 1, k, n), (n,), (n,), (n,)]
    assert all(a is b for a, b in zip(consts, plan.pointwise_constants(name)))
  op0 = plan.crossed_pointwise_operand(W.DECODER_CONV0_POINTWISE)
  assert op0['lda'] == 320 and tuple(op0['a'].shape) == (2, 16, 24, 320)
  assert plan._expr_of(op0['a'], 0, 304) == 'relu(L:%s)' % W.DECODER_CONV0_DEPTHWISE
  assert plan.crossed_pointwise_operand(W.FEATURE_PROJECTION0)['a'].data_ptr() == \
      ch['low_level'].data_ptr()
  assert plan.crossed_pointwise_operand(W.CONCAT_PROJECTION)['a'] is ch['aspp_concat']
  # the trainable layers' accessors answer for their own tables only, and the other way round
  assert sorted(plan.mode.packs) == sorted(W.TRAINABLE_LAYERS)
  with pytest.raises(ValueError, match='crosses'):
    plan.crossed_pointwise_operand(W.DECODER_CONV1_POINTWISE)
  with pytest.raises(ValueError, match='crosses'):
    plan.crossed_depthwise_operand(W.DECODER_CONV1_DEPTHWISE)
  with pytest.raises(ValueError, match='crosses'):
    plan.pointwise_constants(W.DECODER_CONV1_POINTWISE)
  with pytest.raises(EposError, match='no CPU fallback'):                 # a dry run has no device
    trainer.decoder_grads(plan, None, {})

  # the records are records only: the same launches, buffers and order without them
  monkeypatch.setattr(W, 'POINTWISE_CHAIN_LAYERS', {})
  monkeypatch.setattr(W, 'DEPTHWISE_CHAIN_LAYERS', {})
  bare = net.EposNet(ckpt, 2, 64, 96, 2, 4, dry_run=True, model_variant=variant)
  assert not set(want) & set(bare.mode.layer_operands)
  assert _op_list(bare) == _op_list(plan)


def test_bf16_plans_refuse_the_new_accessors():
  from epos_amd import net, weights as W
  ckpt = W.random_init('xception_65', num_objs=2, num_frags=4, seed=0)
  bf16 = net.EposNet(ckpt, 1, 64, 64, 2, 4, dry_run=True, precision='bf16')
  for fn in (bf16.chain_operands, bf16.crossed_depthwise_operand,
             lambda: bf16.crossed_pointwise_operand(W.CONCAT_PROJECTION)):
    with pytest.raises(NotImplementedError, match='bf16'):
      fn()
