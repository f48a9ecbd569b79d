"""Host side of gt_knn_frags > 1 (include/epos_hip.h, "k nearest fragments"): the numpy
restatement tests/helpers/knn_ref.py against the helpers it extends (k = 1, bit for bit), against
torch's fp64 autograd through the structure of the reference's loss.py:186-229,267-303 (k = 2, 3)
and against the reference's own assignment (tests/golden/knn_frags.npz); the host formulas of
epos_amd/loss.py with knn; the two scripts' --gt_knn_frags; the binding of the six entries."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import (heads_dgrad_ref, heads_wgrad_ref, knn_ref, loss_cases,    # noqa: E402
                           loss_grad_ref, loss_ref)

INVALID = -1
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'knn_frags.npz')
C_NAMES = {ctypes.c_int: 'int', ctypes.c_int64: 'int64_t', ctypes.c_double: 'double',
           ctypes.c_float: 'float'}
WEIGHTS = (0.7, 1.3, 100.0)


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
  return a.shape == b.shape and a.dtype == b.dtype and (_bits(a) == _bits(b)).all()


# ------------------------------------------------------------------ golden ---
def test_assignment_equals_the_reference_fixture():
  g = np.load(GOLDEN)
  assert g['xyz'].dtype == np.float32 and g['xyz'].shape == (500, 3)
  for k in (1, 2, 3, 4):
    ids, coords = knn_ref.assign(g['xyz'], g['centers'], g['sizes'], k)
    assert _same(ids, g['ids_k%d' % k]), k
    assert _same(coords, g['coords_k%d' % k]), k          # fp64 subtract and divide, rounded once
  # slot 0 at every k is the nearest fragment
  for k in (2, 3, 4):
    assert (g['ids_k%d' % k][:, 0] == g['ids_k1'][:, 0]).all()


def _generator():
  spec = importlib.util.spec_from_file_location(
      'make_knn_golden', os.path.join(ROOT, 'tests', 'golden', 'make_knn_golden.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_fixture_regenerates_from_the_reference():
  gen = _generator()
  if not os.path.isdir(os.path.join(gen.REFERENCE, 'epos_lib')):
    pytest.skip('the reference is not on this machine')
  saved = dict(sys.modules), list(sys.path)
  try:
    out, gap = gen.generate()
  finally:
    for name in set(sys.modules) - set(saved[0]):
      del sys.modules[name]
    sys.modules.update(saved[0])
    sys.path[:] = saved[1]
  assert gap >= gen.MIN_GAP
  g = np.load(GOLDEN)
  assert sorted(g.files) == sorted(out)
  for name in out:
    assert _same(np.asarray(out[name]), g[name]), name


def test_gt_fields_ties_and_empty_pixels():
  """Two centres equidistant from a pixel: the lower index first; a pixel no instance takes is
  zero in every slot; k == F is every fragment, sorted."""
  centers = np.array([[[1.0, 0, 0], [-1.0, 0, 0], [0, 3.0, 0], [0, 0, 0.5]]])
  sizes = np.array([[2.0, 4.0, 8.0, 16.0]])
  lp = np.zeros((1, 1, 2, 3), np.float32)
  depth = np.array([[[1.0, 0.0]]], np.float32)
  f = knn_ref.gt_fields(depth, lp, None, [1], centers, sizes, 4)
  assert f['frag_label'][0, 0].tolist() == [3, 0, 1, 2]
  assert f['frag_loc'][0, 0, 1].tolist() == [-0.5, 0.0, 0.0]
  assert f['frag_weight'][0, 0].tolist() == [1.0] * 4
  assert f['obj_label'].tolist() == [[1, 0]] and f['instance'].tolist() == [[0, -1]]
  assert not f['frag_label'][0, 1].any() and not f['frag_loc'][0, 1].any()
  assert not f['frag_weight'][0, 1].any()


# ------------------------------------------------------------------ k = 1 ---
@pytest.mark.parametrize('B,P,O,F,seed', [(2, 70, 3, 5, 1), (1, 9, 1, 1, 2), (3, 33, 2, 8, 3)])
def test_k1_equals_the_existing_restatements_bit_for_bit(B, P, O, F, seed):
  c = knn_ref.make_case(B, P, O, F, 1, seed, empty_images=(1,) if B > 1 else ())
  c['gt_obj'][0, P // 2] = O + 3                                   # a bad pixel
  old = knn_ref.squeeze_case(c)
  t_new, t_old = knn_ref.terms(c, 16), loss_cases.ref_terms(loss_ref, old, 16)
  for a, b in zip(t_new, t_old):
    assert _same(a, b)
  sums, counts, _ = t_new
  assert knn_ref.dataset_losses(sums, counts, WEIGHTS, 1) == \
      loss_ref.dataset_losses(sums, counts, WEIGHTS)
  up = np.array([0.3, -1.0, 2.0, 0.5])
  for red in (knn_ref.MEAN, knn_ref.POOLED):
    sc = knn_ref.scales(counts, WEIGHTS, red, 1)
    assert _same(sc, loss_grad_ref.scales(counts, WEIGHTS, red))
    g_new, g_old = knn_ref.grads(c, sc, up), loss_grad_ref.grads(old, sc, up)
    for a, b in zip(g_new, g_old):
      assert _same(a, b)
  for a, b in zip(knn_ref.active_masks(c), loss_grad_ref.active_masks(old)):
    assert (a == b).all()
  cls, frag = knn_ref.classes(c)
  cls_old, frag_old = heads_wgrad_ref.classes(old)
  assert (cls == cls_old).all() and (frag[:, 0][cls > 0] == frag_old[cls > 0]).all()
  rng = np.random.RandomState(seed)
  K = 5
  A = rng.randn(B * P, K).astype(np.float32)
  new = knn_ref.wgrads(A, *g_new, cls, frag)
  ref = heads_wgrad_ref.wgrads(A, *g_old, cls_old, frag_old)
  for d_new, d_old in zip(new, ref):
    for head in heads_wgrad_ref.HEADS:
      pairs = ((d_new[head], d_old[head]),) if isinstance(d_new[head], np.ndarray) else \
          zip(d_new[head], d_old[head])
      for a, b in pairs:
        assert _same(a, b), head
  Ws = [rng.randn(K, n).astype(np.float32) for n in (O + 1, O * F, O * F * 3)]
  for a, b in zip(knn_ref.dgrad(*g_new, *Ws, cls, frag),
                  heads_dgrad_ref.dgrad(*g_old, *Ws, cls_old, frag_old)):
    assert _same(a, b)


# ------------------------------------------------------------------ torch fp64 autograd ---
def _torch_losses(c, b, obj, frag, loc, weights):
  """The three losses of image b as the reference builds them for a batch of one: the object
  cross-entropy over all pixels (weight 0 on ignored ones), and over the foreground the logits
  tiled top_k times, one one-hot row per (pixel, slot), reduce_mean; Huber times the slot
  weight, reduce_mean."""
  P = obj.shape[1]
  knn = c['gt_frag'].shape[-1]
  F = frag.shape[-1]
  g = torch.from_numpy(c['gt_obj'][b].astype(np.int64))
  keep = g != loss_cases.IGNORE
  ce = torch.nn.functional.cross_entropy(obj[b][keep], g[keep], reduction='none')
  l_obj = ce.sum() / P
  fg = torch.nonzero(g * keep >= 1)[:, 0]
  assert fg.numel()                                                 # the cases have foreground
  rows = frag[b][fg, g[fg] - 1]                                     # [n, F]
  rows = rows[:, None, :].repeat(1, knn, 1).reshape(-1, F)          # tf.tile over top_k
  targets = torch.from_numpy(c['gt_frag'][b].astype(np.int64))[fg].reshape(-1)
  tw = torch.from_numpy(c['gt_weight'][b].astype(np.float64))[fg].reshape(-1)
  distrib = torch.zeros((targets.numel(), F), dtype=torch.float64)
  distrib[torch.arange(targets.numel()), targets] = tw
  distrib = distrib / distrib.sum(dim=1, keepdim=True)
  l_cls = (-(distrib * torch.log_softmax(rows, dim=1)).sum(dim=1)).mean()
  pix = fg[:, None].repeat(1, knn).reshape(-1)
  pred = loc[b][pix, g[pix] - 1, targets]                           # [n * k, 3]
  want = torch.from_numpy(c['gt_loc'][b].astype(np.float64))[fg].reshape(-1, 3)
  hub = torch.nn.functional.huber_loss(pred, want, reduction='none', delta=1.0)
  l_loc = (hub * tw[:, None]).mean()
  return weights[0] * l_obj + weights[1] * l_cls + weights[2] * l_loc, l_cls, l_loc


@pytest.mark.parametrize('knn', [2, 3])
def test_restatement_agrees_with_torch_fp64_autograd(knn):
  B, P, O, F = 2, 48, 3, 6
  c = knn_ref.make_case(B, P, O, F, knn, seed=10 + knn)
  c['frag_loc'][0, :, :, :, 0] *= 3.0                               # both Huber branches
  obj, frag, loc = (torch.tensor(c[k].astype(np.float64), requires_grad=True)
                    for k in ('obj_logits', 'frag_logits', 'frag_loc'))
  total = 0.0
  parts = []
  for b in range(B):
    out = _torch_losses(c, b, obj, frag, loc, WEIGHTS)
    total = total + out[0]
    parts.append(out)
  (total / B).backward()
  sums, counts, bad = knn_ref.terms(c, 16)
  assert not bad.any()
  res = knn_ref.dataset_losses(sums, counts, WEIGHTS, knn)
  for b in range(B):
    for name, want in (('total_loss', parts[b][0].item()),
                       ('frag_cls_loss', WEIGHTS[1] * parts[b][1].item()),
                       ('frag_loc_loss', WEIGHTS[2] * parts[b][2].item())):
      assert abs(res['per_image'][b][name] - want) <= 1e-12 * max(1.0, abs(want)), name
  sc = knn_ref.scales(counts, WEIGHTS, knn_ref.MEAN, knn)
  d = knn_ref.grads(c, sc, None, rounded=False)
  for got, t in zip(d, (obj, frag, loc)):
    assert np.abs(got - t.grad.numpy()).max() <= 1e-12
  assert np.abs(d[1]).max() > 1e-4 and np.abs(d[2]).max() > 1e-3


def test_restatement_bad_pixel_rules():
  """One planted pixel per rule, the three new ones included: each counts as bad and adds
  nothing else."""
  B, P, O, F, knn = 1, 12, 2, 4, 2
  base = knn_ref.make_case(B, P, O, F, knn, seed=4, ignore_band=False)
  base['gt_obj'][0, :] = 1
  base['gt_frag'][0, :] = [0, 1]
  base['gt_weight'][0, :] = 1.0
  clean = knn_ref.terms(base, 64)
  assert clean[2][0] == 0 and clean[1][0, 1, 0] == P
  plants = [('gt_obj', (0, 3), O + 1), ('gt_frag', (0, 3, 0), F), ('gt_frag', (0, 3, 1), -1),
            ('gt_weight', (0, 3, 1), 0.0), ('gt_weight', (0, 3, 0), np.inf),
            ('gt_weight', (0, 3, 1), np.nan), ('gt_frag', (0, 3, 1), 0)]
  for key, at, value in plants:
    c = {k: v.copy() for k, v in base.items()}
    c[key][at] = value
    sums, counts, bad = knn_ref.terms(c, 64)
    assert bad[0] == 1 and counts[0, 1, 0] == P - 1, (key, at, value)
    cls, _ = knn_ref.classes(c)
    assert cls[3] == -1 and (np.delete(cls, 3) == 1).all()
    assert not any(m[0, 3].any() for m in knn_ref.active_masks(c))


# ------------------------------------------------------------------ host API ---
def test_image_losses_and_summarize_with_knn_on_hand_tables():
  from epos_amd import loss
  sums = np.array([[[6.0, 0.0, 0.0], [2.0, 8.0, 3.0], [1.0, 4.0, 9.0]]])       # [1, O+1, 3]
  counts = np.array([[[5, 1], [2, 0], [2, 0]]], np.int64)                       # P = 10, n = 4
  w = (1.0, 2.0, 10.0)
  one = loss.image_losses(sums[0], counts[0], w)
  assert one == {'obj_cls_loss': 0.9, 'frag_cls_loss': 2.0 * (12.0 / 4),
                 'frag_loc_loss': 10.0 * (12.0 / 12), 'total_loss': (0.9 + 6.0) + 10.0}
  two = loss.image_losses(sums[0], counts[0], w, knn=2)
  assert two == {'obj_cls_loss': 0.9, 'frag_cls_loss': 2.0 * (12.0 / 8),
                 'frag_loc_loss': 10.0 * (12.0 / 24), 'total_loss': (0.9 + 3.0) + 5.0}
  bad = np.zeros((1,), np.int64)
  res = loss.summarize(sums, counts, bad, w, 2, knn=2)
  assert res['per_image'] == [two] and res['mean'] == two and res['pooled'] == two
  assert res['per_object'][1] == {'frag_cls_loss': 2.0 * (8.0 / 4), 'frag_loc_loss': 10.0 * (3.0 / 12),
                                  'pixels': 2}
  assert res == knn_ref.dataset_losses(sums, counts, w, 2)
  assert loss.summarize(sums, counts, bad, w, 2) == loss.summarize(sums, counts, bad, w, 2, 1)
  assert loss.summarize(sums, counts, bad, w, 2)['mean'] == one
  # two images, one without foreground, against the restatement
  sums2 = np.concatenate([sums, np.array([[[3.0, 0, 0], [0, 0, 0], [0, 0, 0]]])])
  counts2 = np.concatenate([counts, np.array([[[10, 0], [0, 0], [0, 0]]], np.int64)])
  for knn in (1, 3, 4):
    assert loss.summarize(sums2, counts2, np.zeros(2, np.int64), w, 2, knn) == \
        knn_ref.dataset_losses(sums2, counts2, w, knn)
  for knn in (0, 5, 1.5):
    with pytest.raises(ValueError, match='gt_knn_frags'):
      loss.summarize(sums, counts, bad, w, 2, knn=knn)


def test_gt_knn_reads_the_shapes():
  from epos_amd import loss
  z = torch.zeros
  assert loss.gt_knn({'obj_label': z(2, 4, 5), 'frag_label': z(2, 4, 5)}) == 1
  assert loss.gt_knn({'obj_label': z(2, 4, 5), 'frag_label': z(2, 4, 5, 3)}) == 3
  assert loss.gt_knn({'obj_label': z(2, 4, 5), 'frag_label': z(2, 4, 5, 1)}) == 1
  with pytest.raises(ValueError, match='frag_label must have the dimensions'):
    loss.gt_knn({'obj_label': z(2, 4, 5), 'frag_label': z(2, 4, 5, 2, 1)})
  with pytest.raises(ValueError, match='frag_label must have the dimensions'):
    loss.gt_knn({'obj_label': z(2, 4, 5), 'frag_label': z(2, 20)})
  assert loss.MAX_KNN == 4
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  assert '#define EPOS_LOSS_MAX_KNN 4' in header
  rows = open(os.path.join(ROOT, 'epos_amd', 'csrc', 'loss_rows.h')).read()
  assert 'constexpr int LOSS_MAX_KNN = EPOS_LOSS_MAX_KNN;' in rows


# ------------------------------------------------------------------ the scripts ---
@pytest.mark.parametrize('script', ['eval_loss', 'train_heads'])
def test_scripts_take_gt_knn_frags(script, tmp_path, monkeypatch):
  mod = __import__(script)
  monkeypatch.setenv('TF_MODELS_PATH', str(tmp_path))
  monkeypatch.setenv('BOP_PATH', str(tmp_path))
  base = ['--model=toy', '--dataset', 'lm', '--synthetic', '2']
  assert mod.prepare(base)[0].gt_knn_frags == 1                          # the default
  assert mod.prepare(base + ['--gt_knn_frags', '3'])[0].gt_knn_frags == 3
  assert mod.prepare(base + ['--gt_knn_frags=4', '--num_frags', '4'])[0].gt_knn_frags == 4
  for extra in (['--gt_knn_frags', '0'], ['--gt_knn_frags', '-1'], ['--gt_knn_frags', '5'],
                ['--gt_knn_frags', '3', '--num_frags', '2']):
    with pytest.raises(ValueError, match='gt_knn_frags must be in 1\\.\\.'):
      mod.prepare(base + extra)
  (tmp_path / 'toy').mkdir()
  (tmp_path / 'toy' / 'params.yml').write_text('gt_knn_frags: 2\nnum_frags: 8\n')
  args, _ = mod.prepare(base)
  assert args.gt_knn_frags == 2 and args.num_frags == 8
  (tmp_path / 'toy' / 'params.yml').write_text('gt_knn_frags: 2\nnum_frags: 1\n')
  with pytest.raises(ValueError, match='gt_knn_frags must be in 1\\.\\.1'):
    mod.prepare(base)
  (tmp_path / 'toy' / 'params.yml').write_text('gt_knn_frags: two\n')
  with pytest.raises(ValueError, match='gt_knn_frags must be an integer'):
    mod.prepare(base)


# ------------------------------------------------------------------ the binding ---
SIBLINGS = (('epos_gt_fields', 'epos_gt_fields_knn', 11),
            ('epos_loss_terms', 'epos_loss_terms_knn', 13),
            ('epos_loss_reduce', 'epos_loss_reduce_knn', 8),
            ('epos_loss_grads', 'epos_loss_grads_knn', 13),
            ('epos_heads_wgrad_f32', 'epos_heads_wgrad_knn_f32', 16),
            ('epos_heads_dgrad_f32', 'epos_heads_dgrad_knn_f32', 13))


def test_symbols_are_declared_bound_and_exported():
  from epos_amd import _lib
  header = open(os.path.join(ROOT, 'include', 'epos_hip.h')).read()
  assert 'k nearest fragments (csrc/render.hip' in header
  assert '1 <= knn <= min(F, EPOS_LOSS_MAX_KNN)' in header
  assert '#define EPOS_ABI_VERSION 7' in header
  header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)

  def declared(name):
    decl = re.search(r'\bint %s\s*\(([^)]*)\)\s*;' % name, header)
    assert decl, name
    return [a.strip() for a in decl.group(1).split(',')]
  for old, new, at in SIBLINGS:
    a_old, a_new = declared(old), declared(new)
    # the sibling's arguments plus `int knn`, nothing else moved
    assert a_new[:at] + a_new[at + 1:] == a_old and a_new[at] == 'int knn', new
    restype, argtypes = _lib.SYMBOLS[new]
    assert restype is ctypes.c_int and len(argtypes) == len(a_new)
    assert list(argtypes[:at]) + list(argtypes[at + 1:]) == list(_lib.SYMBOLS[old][1])
    for arg, t in zip(a_new, argtypes):
      if '*' in arg:
        assert t is ctypes.c_void_p, arg
      else:
        assert arg.split()[0] == C_NAMES[t], arg
    assert getattr(ctypes.CDLL(_lib.lib_path()), new)        # exported by the built library
  assert _lib.load().epos_abi_version() == 7                 # added without a version change


def test_host_side_refusals_of_knn():
  """knn outside 1..min(F, 4) is refused before anything is launched, in the entry's name."""
  from epos_amd import _lib
  lib = _lib.load()
  p = 4096
  for knn, F in ((0, 8), (5, 8), (3, 2), (-1, 8)):
    msg = b'knn must be in 1..min(num_frags, 4)'
    assert lib.epos_loss_terms_knn(p, 3, p, p, p, p, p, p, 1, 10, 2, F, 255, knn, p, p, p, p,
                                   None) == INVALID
    assert lib.epos_last_error() == b'epos_loss_terms_knn: ' + msg
    assert lib.epos_loss_grads_knn(p, 3, p, p, p, p, p, p, 1, 10, 2, F, 255, knn, p, None, p, 3,
                                   p, p, None) == INVALID
    assert lib.epos_last_error() == b'epos_loss_grads_knn: ' + msg
    assert lib.epos_heads_wgrad_knn_f32(p, 8, 8, p, 3, p, p, p, p, p, p, 1, 10, 2, F, 255, knn, p,
                                        None, p, p, p, p, p, p, p, None) == INVALID
    assert lib.epos_last_error() == b'epos_heads_wgrad_knn_f32: ' + msg
    assert lib.epos_heads_dgrad_knn_f32(p, 3, p, p, p, p, p, p, 1, 10, 2, F, 255, knn, p, None, p,
                                        p, p, 8, 8, None, 8, p, 8, None) == INVALID
    assert lib.epos_last_error() == b'epos_heads_dgrad_knn_f32: ' + msg
    assert lib.epos_gt_fields_knn(p, p, None, p, 1, 4, 4, p, p, 2, F, knn, p, p, p, p, p,
                                  None) == INVALID
    assert lib.epos_last_error() == (b'epos_gt_fields_knn: knn must be in 1..min(num_frags, '
                                     b'EPOS_LOSS_MAX_KNN)')
  for knn in (0, 5):
    assert lib.epos_loss_reduce_knn(p, p, 1, 2, 1.0, 1.0, 1.0, 0, knn, p, p, None) == INVALID
    assert lib.epos_last_error() == b'epos_loss_reduce_knn: knn must be in 1..EPOS_LOSS_MAX_KNN'
  # the old entries refuse in their own names, as before
  assert lib.epos_loss_terms(p, 1, p, p, p, p, p, p, 1, 10, 2, 8, 255, p, p, p, p,
                             None) == INVALID
  assert lib.epos_last_error() == b'epos_loss_terms: ld_obj must be >= num_objs + 1'
