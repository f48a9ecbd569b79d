"""project_to_surface inside the fused pipeline (EposPipeline(project_to_surface=True): closest
points through the mesh index, on the device) against the operator route --
establish_many_to_many(project_to_surface=True) and one fitting call per object, as
infer.process_by_operators runs them -- on the same head tensors, bit for bit; and the two
routes of the infer.py command line."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import mesh_cases                                  # noqa: E402
from tests.test_gpu_order_pipeline import SEED, TARGETS, World, same_poses     # noqa: E402

pytestmark = pytest.mark.gpu


class SurfaceWorld(World):
  """The planted scenes of the ordering tests, with an ellipsoid mesh (1280 faces) per object
  through the store's fragment centres."""

  def __init__(self):
    super().__init__()
    self.store.models = {}
    for o in self.store.dp_model['obj_ids']:
      v, f = mesh_cases.icosphere(3, 1.0, scale=self.store.radii[o])
      self.store.models[o] = {'pts': v, 'faces': f}

  def by_operators(self, pipe, j, prosac=0, K=None, method='progressive_x'):
    import infer
    from epos_amd import fitting
    argv = ['--model', 'm', '--seed', str(SEED), '--use_prosac', str(bool(prosac)),
            '--fitting_method', method, '--project_to_surface', 'true']
    if K is not None:
      argv += ['--max_correspondences', str(K)]
    args = infer.build_parser().parse_args(argv)
    pred = pipe.net.outputs()
    shim = types.SimpleNamespace(
        net=types.SimpleNamespace(forward=lambda imgs, use_graph=False: pred),
        use_graph=False, output_scale=pipe.output_scale, dev=pipe.dev)
    fit = fitting.fit_params(use_prosac=prosac)
    return infer.process_by_operators(shim, self.store, None, self.frames[j], TARGETS[j],
                                      args, fit)[0]


@pytest.fixture(scope='module')
def world():
  return SurfaceWorld()


@pytest.mark.parametrize('prosac,capped,method', [
    (0, False, 'progressive_x'), (0, False, 'opencv_ransac'), (1, True, 'progressive_x')])
def test_fused_projection_equals_operator_route(world, prosac, capped, method):
  from epos_amd import fitting
  K = world.K if capped else None
  pipe = world.pipe(fit_params=fitting.fit_params(use_prosac=prosac), max_correspondences=K,
                    fitting_method=method, project_to_surface=True)
  assert pipe.surface is not None
  assert (pipe.order is not None) == bool(prosac or capped)
  got = world.fused(pipe, 0)
  exp = world.by_operators(pipe, 0, prosac, K, method)
  assert len(got) >= 1
  same_poses(got, exp)
  # the projection moved the points: a pipeline without it fits other poses
  plain = world.fused(world.pipe(fit_params=fitting.fit_params(use_prosac=prosac),
                                 max_correspondences=K, fitting_method=method), 0)
  assert any(np.asarray(p['t']).tobytes() != np.asarray(q['t']).tobytes()
             for p, q in zip(got, plain)) or len(got) != len(plain)


def test_projected_rows_equal_the_sweep(world):
  """After a step the extractor's coord_3d holds, row for row, what the exhaustive sweep makes
  of a plain pipeline's rows (same heads, no projection); nothing else of the rows moved."""
  from epos_amd import corresp
  plain, proj = world.pipe(), world.pipe(project_to_surface=True)
  world.fused(plain, 0)
  world.fused(proj, 0)
  S = plain.corr.S
  base = plain.corr.slot_base.cpu().numpy()[:S + 1]
  assert np.array_equal(base, proj.corr.slot_base.cpu().numpy()[:S + 1])
  n = int(base[-1])
  assert n >= 64
  before = plain.corr.coord_3d.cpu().numpy()[:n]
  after = proj.corr.coord_3d.cpu().numpy()[:n]
  slots, _ = plain.make_slots(TARGETS[0])
  for s, (_, obj) in enumerate(slots):
    lo, hi = int(base[s]), int(base[s + 1])
    m = world.store.models[obj]
    exp = corresp.project_pts_to_model(before[lo:hi], m['pts'], m['faces'])
    assert after[lo:hi].tobytes() == exp.tobytes()
  assert (before != after).any()
  for name in ('coord_2d', 'conf', 'px_id', 'frag_id'):
    assert torch.equal(getattr(plain.corr, name)[:n], getattr(proj.corr, name)[:n]), name


def test_sparse_heads_and_two_batches_enqueued(world):
  """Sparse heads, and queue=2 with the second batch enqueued while the first still runs on
  the same rows: the poses of the dense, one-at-a-time pipeline (= the operator route's)."""
  one = world.pipe(project_to_surface=True)
  exp = []
  for j in range(2):
    exp.append(world.fused(one, j))
    same_poses(exp[j], world.by_operators(one, j))
  sparse = world.pipe(project_to_surface=True, sparse_heads=True)
  for j in range(2):
    same_poses(world.fused(sparse, j), exp[j])
  two = world.pipe(project_to_surface=True, sparse_heads=True, queue=2)
  for j in range(2):
    two.launch(world.images[j], world.Ks, TARGETS[j],
               image_ids=[f.im_id for f in world.frames[j]],
               scene_ids=[f.scene_id for f in world.frames[j]], seed=SEED,
               after_net=world.planter(j))
  got = [two.collect()[0] for _ in range(2)]
  assert sum(len(g) for g in got) >= 2
  for j in range(2):
    same_poses(got[j], exp[j])


def test_default_pipeline_has_no_projector(world):
  """Built without the flag -- meshes in the store or not -- the pipeline has no projection
  stage and fits the poses of a store without meshes."""
  plain = world.pipe()
  assert plain.surface is None
  models, world.store.models = world.store.models, None
  try:
    bare = world.pipe()
    exp = world.fused(bare, 0)
  finally:
    world.store.models = models
  same_poses(world.fused(plain, 0), exp)


def test_missing_mesh_is_refused_at_construction(world):
  models = world.store.models
  try:
    world.store.models = {o: m for o, m in models.items() if o != 2}
    with pytest.raises(ValueError, match='project_to_surface needs model_store.models'):
      world.pipe(project_to_surface=True)
    world.store.models = None
    with pytest.raises(ValueError, match='project_to_surface needs model_store.models'):
      world.pipe(project_to_surface=True)
  finally:
    world.store.models = models


def test_infer_cli_projects_on_the_device_on_request(tmp_path, gpu_children):
  """--project_to_surface through the fused pipeline (--surface_on_device true: sparse heads,
  more than one step in flight) writes the bytes of the default, operator-by-operator run."""
  from epos_amd import ply, synthetic
  store = synthetic.ModelStore(3, 64, seed=0)          # the store infer.py --synthetic builds
  bop = tmp_path / 'bop'
  (bop / 'lm' / 'models_eval').mkdir(parents=True)
  for o in store.dp_model['obj_ids']:
    v, f = mesh_cases.icosphere(2, 1.0, scale=store.radii[o])
    ply.save_ply(ply.model_path(str(bop), 'lm', o, 'eval'), v, f)
  csv, plans = {}, {}
  for on_device in ('false', 'true'):
    d = tmp_path / on_device
    (d / 'toy').mkdir(parents=True)
    (d / 'toy' / 'params.yml').write_text('infer_crop_size: "128,96"\n')
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, 'infer.py'), '--model=toy', '--synthetic', '2',
         '--num_objs', '3', '--dataset', 'lm', '--project_to_surface', 'true',
         '--surface_on_device', on_device],
        env=dict(os.environ, TF_MODELS_PATH=str(d), BOP_PATH=str(bop)), capture_output=True,
        text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = (d / 'toy' / 'infer' / 'estimated-poses.csv').read_text().strip().split('\n')
    csv[on_device] = '\n'.join(','.join(r.split(',')[:-1]) for r in rows)   # last column: time
    plans[on_device] = [l for l in out.stdout.split('\n') if l.startswith('plan: ') and
                        'step(s) in flight' in l][0]
  assert csv['true'] == csv['false']
  assert csv['true'].count('\n') >= 1                 # the header and at least one pose
  steps = lambda line: int(line.split(' step(s) in flight')[0].split()[-1])     # noqa: E731
  assert steps(plans['true']) > 1 and 'sparse heads' in plans['true']
  assert steps(plans['false']) == 1 and 'dense heads' in plans['false']
