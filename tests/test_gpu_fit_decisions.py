"""The HIP pose fit against the C oracle on inputs where each rule of the method DECIDES the
outcome (tests/helpers/fit_decision_cases.py; tests/test_fit_decisions_host.py shows on the
oracle alone that every case is such a witness): through epos_amd.fitting.find6DPoses for every
parameter set of every case, and through the batched device entry for slots that retry, finish
and fail next to each other. The bars are those of test_gpu_corresp_fit.py::_same_as_oracle."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import fit_decision_cases as fd

pytestmark = pytest.mark.gpu

CASES = fd.by_name(fd.CASES)


def _assert_same_as_oracle(got, ref, what):
  assert (got[0] is None) == (ref[0] is None), what
  assert np.array_equal(got[1], ref[1]), what                # labels: bit-exact
  if got[0] is not None:
    assert got[0].shape == ref[0].shape, what
    np.testing.assert_allclose(got[0], ref[0], rtol=0, atol=1e-9, err_msg=str(what))
    np.testing.assert_allclose(got[2], ref[2], rtol=1e-12, err_msg=str(what))


@pytest.mark.parametrize('name', sorted(CASES))
def test_hip_fit_equals_oracle_where_the_rule_decides(name):
  from epos_amd import fitting
  c = CASES[name]
  xy, xyz = fd.scene_of(c.scene)
  for tag, params in fd.param_sets(c):
    got = fitting.find6DPoses(xy, xyz, fd.K, seed=c.seed, max_poses=c.max_k, **params)
    _assert_same_as_oracle(got, fd.oracle_fit(c.scene, c.seed, c.max_k, params), (name, tag))


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr())


def _fit_batch(batch):
  """One call of epos_find6d_poses_device over the batch's slots (rows in image-row order, as
  the plain entry wants them): per slot (poses [3k, 4] or None, labels, scores)."""
  from epos_amd import _lib as L, fitting
  lib = L.load()
  d = 'cuda:0'
  scenes = [fd.scene_of(s[0]) for s in batch.slots]
  S = len(scenes)
  base = np.concatenate([[0], np.cumsum([len(xy) for xy, _ in scenes])]).astype(np.int64)
  cap = int(base[-1])
  c2 = torch.from_numpy(np.concatenate([xy for xy, _ in scenes])).to(d)
  c3 = torch.from_numpy(np.concatenate([xyz for _, xyz in scenes])).to(d)
  sb = torch.from_numpy(base).to(d)
  fit = fitting.fit_params(**batch.shared)
  Ks = torch.from_numpy(np.tile(fd.K.reshape(1, 9), (S, 1))).to(d)
  mm = torch.tensor([s[1] for s in batch.slots], dtype=torch.int32, device=d)
  sd = torch.tensor([s[2] for s in batch.slots], dtype=torch.int64, device=d)
  max_k = batch.max_k
  work = torch.empty(lib.epos_fit_workspace_bytes(S, cap, ctypes.byref(fit), max_k),
                     dtype=torch.uint8, device=d)
  poses = torch.zeros(S, max_k, 12, dtype=torch.float64, device=d)
  scores = torch.zeros(S, max_k, dtype=torch.float64, device=d)
  nm = torch.full((S,), -7, dtype=torch.int32, device=d)
  labels = torch.full((cap,), -5, dtype=torch.int32, device=d)
  L.check(lib.epos_find6d_poses_device(
      _ptr(c2), _ptr(c3), _ptr(sb), S, cap, _ptr(Ks), _ptr(mm), _ptr(sd), ctypes.byref(fit),
      max_k, _ptr(work), _ptr(poses), _ptr(scores), _ptr(nm), _ptr(labels),
      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'epos_find6d_poses_device')
  torch.cuda.synchronize()
  poses, scores, nm, labels = (t.cpu().numpy() for t in (poses, scores, nm, labels))
  out = []
  for s in range(S):
    k = int(nm[s])
    assert 0 <= k <= max_k, (s, k)
    P = None
    if k:
      P = np.concatenate([poses[s, :k, :9].reshape(k, 3, 3), poses[s, :k, 9:, None]],
                         axis=2).reshape(3 * k, 4)
    out.append((P, labels[base[s]:base[s + 1]], scores[s, :k]))
  return out


@pytest.mark.parametrize('name', [b.name for b in fd.BATCHES])
def test_slots_of_one_call_equal_their_single_calls(name):
  """Per-slot state of the batched launch (tries, last_new, done): every slot of the call
  equals its own single call byte for byte, and the oracle at the usual bars."""
  from epos_amd import fitting
  batch = {b.name: b for b in fd.BATCHES}[name]
  got = _fit_batch(batch)
  counts = []
  for s, (scene, mm, seed) in enumerate(batch.slots):
    params = dict(batch.shared, max_model_number=mm)
    xy, xyz = fd.scene_of(scene)
    one = fitting.find6DPoses(xy, xyz, fd.K, seed=seed, max_poses=batch.max_k, **params)
    assert (got[s][0] is None) == (one[0] is None), (name, s)
    assert got[s][1].tobytes() == one[1].tobytes(), (name, s)
    assert got[s][2].tobytes() == one[2].tobytes(), (name, s)
    if one[0] is not None:
      assert got[s][0].tobytes() == one[0].tobytes(), (name, s)
    _assert_same_as_oracle(got[s], fd.oracle_fit(scene, seed, batch.max_k, params), (name, s))
    counts.append(fd.num_models(got[s]))
  if name == 'none_next_to_three':
    assert counts[:2] == [0, 3], counts


def test_parameters_the_entry_cannot_honour_are_refused():
  """validate_fit_params: a refusal with a message, never another result."""
  from epos_amd import _lib as L, fitting
  xy, xyz = fd.scene_of(fd.FEW_10)
  for kw, text in (({'max_iters': 0}, b'max_iters'), ({'gc_sweeps': 17}, b'gc_sweeps'),
                   ({'gc_sweeps': -1}, b'gc_sweeps'), ({'pearl_iters': 9}, b'pearl_iters')):
    with pytest.raises(L.EposError):
      fitting.find6DPoses(xy, xyz, fd.K, **kw)
    assert text in L.load().epos_last_error(), kw
