"""CPU-only checks of the fit's decision table (tests/helpers/fit_decision_cases.py): the oracle
alone. Every case is a WITNESS -- the oracle's result for the base and for each variant differ,
so the rule the case is about decides what leaves the stage (or, for the `equal` cases, the
variant gives the base's result: a rule that switches a step off) -- and every field of the
parameter struct has one. This is what keeps tests/test_gpu_fit_decisions.py, which compares the
HIP fit with the oracle on the same table, from passing on inputs where a rule never decides."""
import numpy as np
import pytest

from helpers import fit_decision_cases as fd

CASES = fd.by_name(fd.CASES)
BATCHES = {b.name: b for b in fd.BATCHES}


def _fit(case, params):
  return fd.oracle_fit(case.scene, case.seed, case.max_k, params)


def test_table_is_well_formed():
  from oracle import pnp_ref
  assert fd.FIELDS == tuple(f for f, _ in pnp_ref.PnpRefParams._fields_)
  from epos_amd import _lib
  assert fd.FIELDS == tuple(f for f, _ in _lib.FitParams._fields_)
  assert len(CASES) == len(fd.CASES)
  for c in fd.CASES:
    n = len(fd.scene_of(c.scene)[0])
    assert 24 <= n <= 3000, (c.name, n)                # a few dozen to about 3000 rows
    assert c.variants and set(c.base) <= set(fd.FIELDS)
    moved = fd.moved_fields(c)
    assert 1 <= len(moved) <= (3 if c.equal else 1), (c.name, moved)
    for v in c.variants + c.extra:
      assert set(v) <= set(moved) and any(c.base.get(f, None) != v[f] for f in v), (c.name, v)
    tags = [t for t, _ in fd.param_sets(c)]
    assert len(set(tags)) == len(tags), c.name


@pytest.mark.parametrize('name', sorted(CASES))
def test_case_is_a_witness(name):
  c = CASES[name]
  base = _fit(c, c.base)
  for v in c.variants:
    res = _fit(c, dict(c.base, **v))
    if c.equal:
      assert fd.same_result(base, res), (name, v)
      assert res[0] is not None and (res[0] == base[0]).all() and (res[2] == base[2]).all()
    else:
      assert not fd.same_result(base, res), (name, v, fd.num_models(base))


def test_every_field_has_a_witness():
  """... among the cases that must DIFFER, scaling_from_millimeters included (the `equal` cases
  do not count)."""
  seen = set()
  for c in fd.CASES:
    if not c.equal:
      seen.update(fd.moved_fields(c))
  assert seen == set(fd.FIELDS), sorted(set(fd.FIELDS) - seen)


def test_what_the_cases_are_named_for_happens():
  """The model counts behind the acceptance and termination cases, as the table's comments
  state them."""
  n = lambda name, **kw: fd.num_models(_fit(CASES[name], dict(CASES[name].base, **kw)))  # noqa: E731
  assert n('min_triangle_area') == 1 and n('min_triangle_area', min_triangle_area=1e7) == 0
  for name, count in (('min_point_number_10_inliers', 10), ('min_point_number_5_inliers', 5)):
    c = CASES[name]                                    # exactly `count` inliers: accepted at it
    assert (_fit(c, dict(c.base, min_point_number=3))[1] == 0).sum() == count
    assert n(name, min_point_number=count) == 1 and n(name, min_point_number=count + 1) == 0
    assert {'min_point_number': count} in c.variants + c.extra
    assert count + 1 in [v['min_point_number'] for v in c.variants] + [6]   # 6: the base
  c = CASES['max_model_number_for_optimization']       # as many instances as the cap: refined
  assert {'max_model_number_for_optimization': fd.num_models(_fit(c, c.base))} in c.extra
  assert n('min_coverage') == 1 and n('min_coverage', min_coverage=0.0) == 3
  assert n('max_tanimoto_similarity') == 3
  assert n('max_tanimoto_similarity', max_tanimoto_similarity=0.2) == 1
  for mi in (2, 3, 4, 5):                               # retried and found / stopped
    name = 'conf_retry_%d_iters' % mi
    assert CASES[name].base['max_iters'] == mi
    assert n(name) == 1 and n(name, conf=1e-9) == 0
    # the retry, not the first round, found it: a single-instance search never retries
    assert n(name, max_model_number=1) == 0
  # the bound itself: one retry allowed / needed, two needed
  assert fd.CONF_NO_RETRY < 1 - (1 - 0.2 ** 3) ** 5 < fd.CONF_ONE_RETRY < 1 - (1 - 0.2 ** 3) ** 10
  for name, one_retry in (('conf_bound_first_retry', 1), ('conf_bound_second_retry', 0)):
    assert CASES[name].base['min_point_number'] * 5 == len(fd.scene_of(CASES[name].scene)[0])
    assert n(name) == 1 and n(name, conf=fd.CONF_NO_RETRY) == 0
    assert n(name, conf=fd.CONF_ONE_RETRY) == one_retry
  name = 'conf_retry_after_first_instance'
  assert n(name) == 2 and n(name, conf=1e-9) == 1
  # what the joint_* cases move acts through the joint refinement alone (but the radius and
  # the threshold, which the proposals read too)
  for f in ('gc_sweeps', 'spatial_coherence_weight', 'scaling_from_millimeters'):
    c = CASES['joint_' + f]
    off = dict(c.base, pearl_iters=0)
    for v in c.variants:
      assert fd.same_result(_fit(c, off), _fit(c, dict(off, **v))), (f, v)
  # the bound stops at one sample exactly: one fewer or one more gives another result
  for name, (same, other) in fd.BOUND_STOPS.items():
    c = CASES[name]
    bounded = _fit(c, dict(c.base, **c.variants[0]))
    assert abs(same - other) == 1
    assert fd.same_result(bounded, _fit(c, dict(c.base, max_iters=same))), name
    assert not fd.same_result(bounded, _fit(c, dict(c.base, max_iters=other))), name
  # radius 40 of joint_neighborhood_ball_radius: points with more neighbours than the device's
  # neighbour lists hold (4 sub-lists of 160 entries, docs/fitting.md)
  c = CASES['joint_neighborhood_ball_radius']
  assert {'neighborhood_ball_radius': 40.0} in c.variants
  xy, xyz = fd.scene_of(c.scene)
  p5 = np.concatenate([xy, 0.1 * xyz], 1)
  deg = np.array([(((p5 - p) ** 2).sum(1) <= 40.0 ** 2).sum() - 1 for p in p5[::7]])
  assert (deg > 4 * 160).mean() > 0.1 and deg.max() < 1000
  # the step the `equal` case switches off does decide on that scene when it runs
  c = CASES['off_by_its_own_rule']
  assert not fd.same_result(_fit(c, c.base), _fit(c, dict(c.base, gc_sweeps=2)))
  # the joint refinement moves poses or labels of the two-instance scene (it is no fixed point)
  c = CASES['pearl_iters']
  assert fd.num_models(_fit(c, c.base)) == fd.num_models(_fit(c, dict(c.base, pearl_iters=0))) == 4


def _inliers(P, i, xy, xyz, thr=4.0):
  """Inlier mask of instance i of the poses [3k, 4], in numpy."""
  from helpers import fit_scenes as fs
  r, z = fs.reproj_residuals(P[3 * i:3 * i + 3, :3], P[3 * i:3 * i + 3, 3], fd.K, xy, xyz)
  return ((r * r).sum(1) < thr * thr) & (z > 0)


def test_the_set_ratios_the_acceptance_cases_rest_on():
  """Which count stands in which ratio, restated in numpy on the oracle's poses (without the
  joint refinement, so that poses and labels are those of the acceptance): the Tanimoto cases
  accept and reject by intersection / UNION, the retry case by NEW rows / unexplained rows."""
  c = CASES['max_tanimoto_similarity']
  xy, xyz = fd.scene_of(c.scene)
  P, _, _ = _fit(c, dict(c.base, pearl_iters=0))
  a, b = _inliers(P, 0, xy, xyz), _inliers(P, 1, xy, xyz)
  inter, values = float((a & b).sum()), sorted(v['max_tanimoto_similarity']
                                                for v in c.variants + c.extra)
  assert values == [0.2, 0.3, 0.35, 0.5]
  assert 0.3 < inter / (a | b).sum() < 0.35 < inter / a.sum() < 0.5 < inter / b.sum()
  assert [fd.num_models(_fit(c, dict(c.base, max_tanimoto_similarity=t))) for t in values] == \
      [1, 1, 3, 3]
  c = CASES['conf_bound_counts_new_rows']
  assert c.base['pearl_iters'] == 0 and c.base['max_iters'] == 3
  xy, xyz = fd.scene_of(c.scene)
  P, lab, _ = _fit(c, dict(c.base, **c.variants[0]))          # stops at the first failure
  assert fd.num_models((P, lab, None)) == 2 and fd.num_models(_fit(c, c.base)) == 3
  n_inl, n_new, n_left = _inliers(P, 1, xy, xyz).sum(), (lab == 1).sum(), (lab < 0).sum()
  keep_on = 1.0 - c.base['conf']
  assert n_new < n_inl < n_left
  assert (1 - (n_new / n_left) ** 3) ** (3 * 3) > keep_on + 0.1     # a third retry still runs
  assert (1 - (n_inl / n_left) ** 3) ** 3 < keep_on - 0.02          # ... not even a first


def _slot_fit(batch, slot, **kw):
  scene, mm, seed = slot
  return fd.oracle_fit(scene, seed, batch.max_k, dict(batch.shared, max_model_number=mm, **kw))


def test_batches_hold_what_they_are_for():
  b = BATCHES['retry']
  counts = [fd.num_models(_slot_fit(b, s)) for s in b.slots]
  # slots whose outcome the retry decided (stopping at the first failure gives another result)
  retried = [not fd.same_result(_slot_fit(b, s), _slot_fit(b, s, conf=1e-9)) for s in b.slots]
  assert sum(retried) >= 2 and not all(retried), retried
  assert len(set(counts)) >= 3, counts                  # the slots end in different rounds
  assert len({s[2] for s in b.slots}) > 2 and len({s[1] for s in b.slots}) == 3
  b = BATCHES['none_next_to_three']
  counts = [fd.num_models(_slot_fit(b, s)) for s in b.slots]
  assert counts[:2] == [0, 3] and 1 in counts, counts
  for b in fd.BATCHES:
    assert b.shared and set(b.shared) <= set(fd.FIELDS)
    for s in b.slots:                                   # the plain entry wants rows in row order
      xy = fd.scene_of(s[0])[0]
      assert (xy[1:, 1] >= xy[:-1, 1]).all()
