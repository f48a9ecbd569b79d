"""Case table of the pose fit's decisions (docs/fitting.md (f), steps 1-6), in the style of
tests/helpers/heads_cases.py: ONE table, read by tests/test_fit_decisions_host.py (the oracle
alone, no GPU) and tests/test_gpu_fit_decisions.py (HIP against the oracle).

A case is about one rule of the method. It holds a seeded scene, the call's seed and max_k, a
BASE parameter set and VARIANTS that differ from the base in the one field (or the one named
pair of fields) the case moves. A case is a WITNESS when the oracle's result for the base and
for each variant differ -- another number of models, another label vector or another pose:
there the rule decides what leaves the stage, so an implementation that gets it wrong cannot
agree with the oracle on both. The cases with equal = True pin the opposite: the variant must
give the base's result (a rule that switches a step off). `extra` parameter sets are compared
on the device like the others but carry no witness condition (max_iters = 401: another grid
shape, possibly the same winner).

Parameter sets are keyword dictionaries of oracle.pnp_ref.default_params, which
epos_amd.fitting.find6DPoses takes under the same names. Pure numpy + the C oracle.
"""
import collections
import functools

import numpy as np

from . import fit_scenes as fs

K = fs.K_YCBV

# the fields of EposFitParams / PnpRefParams, in declaration order
FIELDS = ('threshold', 'neighborhood_ball_radius', 'spatial_coherence_weight',
          'scaling_from_millimeters', 'max_tanimoto_similarity', 'conf', 'proposal_engine_conf',
          'min_coverage', 'min_triangle_area', 'max_iters', 'min_point_number',
          'max_model_number', 'max_model_number_for_optimization', 'use_prosac', 'lo_iters',
          'gc_sweeps', 'pearl_iters')


# ------------------------------------------------------------------------------ scenes ---
def _frozen(*arrays):
  out = tuple(np.ascontiguousarray(a, np.float64) for a in arrays)
  for a in out:
    a.setflags(write=False)                 # shared among the tests: nobody edits a scene
  return out


@functools.lru_cache(maxsize=None)
def dense(rs, sigma3d, sym, outlier, shuffled=False):
  """One ellipsoid under a random pose, as tests/test_gpu_corresp_fit.py draws it: EPOS-like
  rows in raster order (fit_scenes.dense_scene); shuffled: in a seeded random order."""
  rng = np.random.RandomState(rs)
  R = fs.rand_rot(rng)
  t = np.array([rng.uniform(-100, 100), rng.uniform(-60, 60), rng.uniform(600, 1000)])
  xy, xyz, _, _ = fs.dense_scene(rng, [(R, t)], sigma3d=sigma3d, sym=sym, outlier=outlier)
  if shuffled:
    perm = rng.permutation(len(xy))
    xy, xyz = xy[perm], xyz[perm]
  return _frozen(xy, xyz)


@functools.lru_cache(maxsize=None)
def cloud(rs, n, outlier, sigma, best_first=False):
  """n points of a uniform cloud under a random pose, projected with `sigma` pixels of noise,
  the first n * outlier of them moved to random pixels; sorted by image row (stable), so that
  the plain device entry takes the rows as they are. best_first: not sorted -- the inliers
  come first, as in a confidence order that is worth its name (PROSAC)."""
  rng = np.random.RandomState(rs)
  R = fs.rand_rot(rng)
  t = np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(600, 1200)])
  X = rng.uniform(-60, 60, (n, 3))
  p = (X @ R.T + t) @ K.T
  p = p[:, :2] / p[:, 2:]
  p += rng.standard_normal(p.shape) * sigma
  no = int(n * outlier)
  p[:no] = rng.uniform(0, [640, 480], (no, 2))
  order = np.arange(n)[::-1] if best_first else np.argsort(p[:, 1], kind='stable')
  return _frozen(p[order], X[order])


@functools.lru_cache(maxsize=None)
def two_instances(shuffled=False):
  """The scene of test_two_close_instances_of_a_symmetric_object (test_gpu_corresp_fit.py);
  shuffled: in a seeded random order."""
  rng = np.random.RandomState(77)
  Ra, Rb = fs.rand_rot(rng), fs.rand_rot(rng)
  insts = [(Ra, np.array([-38.0, 10.0, 760.0])), (Rb, np.array([42.0, -5.0, 790.0]))]
  xy, xyz, _, _ = fs.dense_scene(rng, insts, sigma3d=0.7, sym=1.0, outlier=0.2)
  if shuffled:
    perm = rng.permutation(len(xy))
    xy, xyz = xy[perm], xyz[perm]
  return _frozen(xy, xyz)


def scene_of(spec):
  """spec = (builder, arguments...): (xy [n, 2], xyz [n, 3]), read-only and cached."""
  return spec[0](*spec[1:])


# ------------------------------------------------------------------------------- cases ---
_Case = collections.namedtuple('_Case', 'name decision scene seed max_k base variants equal extra')


def Case(name, decision, scene, seed, variants, base=None, max_k=4, equal=False, extra=()):
  return _Case(name, decision, tuple(scene), seed, max_k, dict(base or {}),
               tuple(dict(v) for v in variants), equal, tuple(dict(v) for v in extra))


def by_name(table):
  d = {c.name: c for c in table}
  assert len(d) == len(table), 'duplicate case names'
  return d


def moved_fields(case):
  return sorted({f for v in case.variants for f in v})


def param_sets(case):
  """Every parameter set of a case, the base first: [(tag, keyword dictionary)]."""
  def tag(v):
    return ','.join('%s=%s' % (f, v[f]) for f in sorted(v))
  return ([('base', dict(case.base))] +
          [(tag(v), dict(case.base, **v)) for v in case.variants + case.extra])


def _vary(field, values):
  return [{field: v} for v in values]


PLAIN = (dense, 40, 1.0, 0.5, 0.3)            # an EPOS-like scene the defaults fit well
PLAIN_B = (dense, 41, 1.0, 0.5, 0.3)
PLAIN_C = (dense, 42, 1.0, 0.5, 0.3)
NOISY_A = (dense, 600, 3.0, 0.5, 0.5)         # 3 mm of noise, half the pixels with an outlier:
NOISY_B = (dense, 603, 3.0, 0.5, 0.5)         # the refit on the labelled set IS kept here
FEW_10 = (cloud, 700, 24, 0.6, 1.0)           # 24 rows, 10 of them inliers
FEW_5 = (cloud, 700, 24, 0.8, 1.0)            # 24 rows, 5 of them inliers
OVERLAP = (cloud, 800, 1500, 0.3, 3.0)        # one instance, 3 px of noise: a second proposal
                                              # finds the same instance again
WEAK = [(cloud, 900 + s, 300, 0.75, 1.0) for s in (4, 6, 1, 2)]   # 75 of 300 rows inliers
TWO = (two_instances,)
# a model of 60 of 300 rows has w^3 = 0.008: with 5 samples per round the bound (1 - w^3)^(5 tries)
# > 1 - conf lets a first retry run iff conf > 0.0394 and a second iff conf > 0.0772
CONF_NO_RETRY, CONF_ONE_RETRY = 0.03, 0.0583

CASES = (
    # ---- 1. proposal
    [Case('threshold', 'MSAC threshold', PLAIN, 0, _vary('threshold', [2.0, 8.0])),
     # ceil(max_iters / 4) workgroups: a ragged last one (1, 2, 3, 5, 7), one workgroup more
     # than the default (401), a table shorter and longer than the default's 1600 scores
     Case('max_iters', 'hypothesis count and grid shape', PLAIN, 0,
          _vary('max_iters', [1, 2, 3, 5, 7, 100, 1000]), extra=_vary('max_iters', [401])),
     Case('max_iters_b', 'hypothesis count and grid shape', PLAIN_C, 2,
          _vary('max_iters', [1, 2, 3, 5, 7, 100]), extra=_vary('max_iters', [401, 1000])),
     # the bound's sequential scan over a table that is not 1600 entries long
     Case('max_iters_bounded', 'hypothesis count and grid shape', PLAIN_C, 2,
          _vary('max_iters', [3, 5]), base={'proposal_engine_conf': 0.99},
          extra=_vary('max_iters', [100, 401, 1000])),   # the bound stops before the 100th
     Case('min_triangle_area', 'degenerate-sample skip', PLAIN, 0,
          _vary('min_triangle_area', [2000.0, 1e7])),          # 1e7: no sample survives
     Case('use_prosac', 'PROSAC prefix', PLAIN + (True,), 0, _vary('use_prosac', [1])),
     Case('use_prosac_7_iters', 'PROSAC prefix', PLAIN_B + (True,), 1,
          _vary('use_prosac', [1]), base={'max_iters': 7}),
     # the prefix of a compacted active list: the second round of a two-instance search
     Case('use_prosac_two_rounds', 'PROSAC prefix', TWO + (True,), 5, _vary('use_prosac', [1]),
          base={'max_model_number': 2}, max_k=5),
     # 24 rows, 50 samples: the prefix ceil(24 (it + 1) / 50) stays below 6 for ten samples,
     # where it is min_point_number rows instead (17 inliers: the support test does not bind)
     Case('use_prosac_prefix_floor', 'PROSAC prefix', (cloud, 702, 24, 0.3, 1.0, True), 1,
          _vary('min_point_number', [3, 8, 10]), base={'use_prosac': 1, 'max_iters': 50}),
     Case('proposal_engine_conf', 'early stop of the proposal loop', PLAIN_C, 2,
          _vary('proposal_engine_conf', [0.99, 0.5])),
     # the sample at which the bound stops, to the sample (BOUND_STOPS): the winner is the last
     # sample drawn before the stop / the first sample not drawn any more would have won
     Case('bound_stops_behind_its_winner', 'early stop of the proposal loop', PLAIN_B, 0,
          _vary('proposal_engine_conf', [0.99])),
     Case('bound_stops_before_a_better_sample', 'early stop of the proposal loop', PLAIN_C, 1,
          _vary('proposal_engine_conf', [0.99]))] +
    # ---- 2. local optimisation (i)
    [Case('lo_iters', 'LO (i) refits', PLAIN, 0, _vary('lo_iters', [0, 1, 2])),
     Case('lo_iters_b', 'LO (i) refits', PLAIN_B, 1, _vary('lo_iters', [0, 1, 2]))] +
    # ---- 3. local optimisation (ii): the labelling feeds a refit that is kept
    [Case('gc_sweeps', 'LO (ii) labelled refit', NOISY_A, 0, _vary('gc_sweeps', [0, 1, 5]),
          base={'neighborhood_ball_radius': 9.0}),
     Case('gc_sweeps_b', 'LO (ii) labelled refit', NOISY_B, 3, _vary('gc_sweeps', [0, 1, 5]),
          base={'spatial_coherence_weight': 0.4, 'neighborhood_ball_radius': 5.0}),
     Case('spatial_coherence_weight', 'LO (ii) labelled refit', NOISY_B, 3,
          _vary('spatial_coherence_weight', [0.4, 0.8]),
          base={'neighborhood_ball_radius': 5.0}),
     Case('neighborhood_ball_radius', 'LO (ii) labelled refit', NOISY_A, 0,
          _vary('neighborhood_ball_radius', [5.0, 9.0])),
     Case('scaling_from_millimeters', 'LO (ii) labelled refit', NOISY_A, 0,
          _vary('scaling_from_millimeters', [1.0, 10.0]),
          base={'spatial_coherence_weight': 0.4, 'neighborhood_ball_radius': 5.0}),
     # lambda = 0 or radius = 0 IS gc_sweeps = 0 (the oracle's `> 0.0` guards); the case
     # 'gc_sweeps' shows that the step decides on this scene when it runs
     Case('off_by_its_own_rule', 'step (ii) off by its own rule', NOISY_A, 0,
          [{'gc_sweeps': 2, 'spatial_coherence_weight': 0.0},
           {'gc_sweeps': 2, 'neighborhood_ball_radius': 0.0}],
          base={'gc_sweeps': 0, 'neighborhood_ball_radius': 9.0}, equal=True)] +
    # ---- 4. acceptance (a model with exactly min_point_number inliers is accepted: 10 / 11, 5 / 6)
    [Case('min_point_number_10_inliers', 'minimum support', FEW_10, 0,
          _vary('min_point_number', [11, 12, 20]), extra=_vary('min_point_number', [3, 10])),
     Case('min_point_number_5_inliers', 'minimum support', FEW_5, 0,
          _vary('min_point_number', [3, 4, 5]), extra=_vary('min_point_number', [7, 12])),
     Case('min_coverage', 'coverage rejection', OVERLAP, 0, _vary('min_coverage', [0.0]),
          base={'max_model_number': 3}),
     # the second proposal shares 0.31 of the union with the first instance, 0.36 of the first's
     # inliers and 0.70 of its own: 0.35 and 0.5 accept it -- with the union as denominator only
     Case('max_tanimoto_similarity', 'Tanimoto rejection', OVERLAP, 0,
          _vary('max_tanimoto_similarity', [0.2, 0.3]),
          base={'max_model_number': 3, 'min_coverage': 0.0, 'max_tanimoto_similarity': 1.01},
          extra=_vary('max_tanimoto_similarity', [0.35, 0.5])),
     Case('max_model_number', 'instance count', TWO, 5,
          _vary('max_model_number', [2, 4, -1]), max_k=5)] +
    # ---- 5. Progressive-X termination: the first round fails; conf = 0.5 retries (and finds the
    #         instance), conf = 1e-9 stops
    [Case('conf_retry_%d_iters' % mi, 'retry after a failed round, and the conf bound', sc,
          seed, _vary('conf', [1e-9]), base={'max_model_number': 2, 'max_iters': mi})
     for mi, sc, seed in zip((2, 3, 4, 5), WEAK, (4, 6, 1, 2))] +
    # the bound itself, before any instance (its ratio is min_point_number / unexplained rows):
    # found by the FIRST retry -- conf just above the bound of one try gives the base's result;
    # found by the SECOND retry -- that conf stops one round too early
    [Case('conf_bound_first_retry', 'retry after a failed round, and the conf bound',
          (cloud, 902, 300, 0.75, 1.0), 2, _vary('conf', [1e-9, CONF_NO_RETRY]),
          base={'max_model_number': 2, 'max_iters': 5, 'min_point_number': 60},
          extra=_vary('conf', [CONF_ONE_RETRY])),
     Case('conf_bound_second_retry', 'retry after a failed round, and the conf bound',
          (cloud, 901, 300, 0.75, 1.0), 1, _vary('conf', [1e-9, CONF_NO_RETRY, CONF_ONE_RETRY]),
          base={'max_model_number': 2, 'max_iters': 5, 'min_point_number': 60}),
     # ... and after an accepted instance (its ratio is that instance's new rows / unexplained)
     Case('conf_retry_after_first_instance', 'retry after a failed round, and the conf bound',
          TWO, 1, _vary('conf', [1e-9]),
          base={'max_model_number': 2, 'max_iters': 5, 'min_point_number': 100}, max_k=5),
     # the second instance has 121 NEW rows among its 324 inliers, 739 rows stay unexplained:
     # three failed rounds are retried at conf = 0.2 only if the ratio counts the new rows
     Case('conf_bound_counts_new_rows', 'retry after a failed round, and the conf bound',
          OVERLAP, 2, _vary('conf', [1e-9]), max_k=5,
          base={'max_model_number': 4, 'min_coverage': 0.0, 'max_iters': 3, 'conf': 0.2,
                'pearl_iters': 0})] +
    # ---- 6. joint refinement
    [Case('pearl_iters', 'joint refinement moves the result', TWO, 5,
          _vary('pearl_iters', [0, 8]), base={'max_model_number': 4}, max_k=5),
     Case('max_model_number_for_optimization', 'joint refinement moves the result', TWO, 5,
          _vary('max_model_number_for_optimization', [1, 3]), base={'max_model_number': 4},
          max_k=5, extra=_vary('max_model_number_for_optimization', [4]))] +   # 4 are found
    # what the joint refinement reads of the other fields (with pearl_iters = 0 the sweeps, the
    # weight and the scale change nothing on this scene: tests/test_fit_decisions_host.py).
    # Radius 40: a fifth of the points have more neighbours than the four sub-lists of 160 entries
    # hold, so the lists overflow and the passes walk the windows instead
    [Case('joint_' + f, 'joint refinement: sweeps, graph, weight, threshold', TWO, 5,
          _vary(f, vals), base={'max_model_number': 4}, max_k=5, extra=_vary(f, more))
     for f, vals, more in (('gc_sweeps', [1, 0], [5]),
                           ('neighborhood_ball_radius', [9.0, 40.0], []),
                           ('spatial_coherence_weight', [0.4, 0.8], []),
                           ('scaling_from_millimeters', [1.0], []),
                           ('threshold', [2.0, 8.0], []))])

# case -> (max_iters that gives the bounded result with the bound off, its neighbour that does not)
BOUND_STOPS = {'bound_stops_behind_its_winner': (30, 29),
               'bound_stops_before_a_better_sample': (89, 90)}

# Slots of ONE call of the batched device entry under one shared, non-default parameter set;
# (scene, max_models, seed) per slot. 'retry': slots whose first round fails and is retried sit
# next to slots that have finished (per-slot tries / last_new / done). 'none_next_to_three': a
# slot without a model next to one that finds three.
Batch = collections.namedtuple('Batch', 'name shared max_k slots')

BATCHES = (
    Batch('retry', {'max_iters': 5, 'conf': 0.5, 'min_coverage': 0.0}, 3,
          ((WEAK[0], 2, 4), (OVERLAP, 2, 1), (WEAK[2], 3, 7), (PLAIN, 1, 0), (WEAK[1], 3, 7),
           (OVERLAP, 3, 0), (WEAK[2], 2, 1), (PLAIN, 3, 0))),
    Batch('none_next_to_three', {'min_coverage': 0.0}, 3,
          ((FEW_5, 1, 0), (OVERLAP, 3, 0), (FEW_5, 3, 1), (PLAIN, 1, 0))),
)


# ------------------------------------------------------------------------------ oracle ---
def oracle_max_k(params, max_k):
  """The max_k epos_amd.fitting.find6DPoses derives from (max_model_number, max_poses)."""
  mm = params.get('max_model_number', 1)
  return max_k if mm < 0 else max(1, min(mm, max_k))


_results = {}


def oracle_fit(scene, seed, max_k, params):
  """(poses [3k, 4] or None, labels, scores) of the oracle; computed once per process."""
  from oracle import pnp_ref
  key = (scene, seed, max_k, tuple(sorted(params.items())))
  if key not in _results:
    xy, xyz = scene_of(scene)
    res = pnp_ref.find6DPoses(xy, xyz, K, params=pnp_ref.default_params(**params), seed=seed,
                              max_k=oracle_max_k(params, max_k))
    for a in res:
      if a is not None:
        a.setflags(write=False)
    _results[key] = res
  return _results[key]


def num_models(res):
  return 0 if res[0] is None else res[0].shape[0] // 3


def same_result(a, b):
  """Not a witness: the same number of models, label vector and poses."""
  if num_models(a) != num_models(b) or not np.array_equal(a[1], b[1]):
    return False
  return num_models(a) == 0 or np.array_equal(a[0], b[0])
