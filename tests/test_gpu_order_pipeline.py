"""use_prosac / max_correspondences inside the fused pipeline (device-side confidence order)
against infer.process_by_operators (host sort, one fitting call per object) on the same head
tensors -- bit for bit -- and the two routes of the infer.py command line."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

O, F, B, H, W_ = 3, 64, 2, 96, 128
CAM = np.array([[300., 0, 64], [0, 300., 48], [0, 0, 1]])
TARGETS = [[{1: 1, 3: 1}, {2: 1}], [{2: 1}, {1: 1, 2: 1}]]     # two batches
SEED = 3


class World(object):
  """Checkpoint, model store, two batches of frames and the planted head values of each."""

  def __init__(self):
    from epos_amd import _lib, synthetic, weights
    self.lib = _lib.load()
    self.ckpt = weights.random_init(num_objs=O, seed=5, randomize_bn=True)
    self.store = synthetic.ModelStore(O, F, seed=0)
    self.Ks = np.tile(CAM, (B, 1, 1))
    self.images, self.frames, self.plants = [], [], []
    plain = self.pipe()
    for j, tg in enumerate(TARGETS):
      idx = [10 * j + b for b in range(B)]
      self.images.append(torch.from_numpy(
          np.stack([synthetic.image(i, H, W_) for i in idx])).cuda())
      self.frames.append([types.SimpleNamespace(scene_id=1, im_id=i, K=CAM, targets=tg[b])
                          for b, i in enumerate(idx)])
      scenes = [synthetic.planted_scene(i, self.store, tg[b], CAM, plain.net.out_h,
                                        plain.net.out_w, O, F, image_in_batch=b,
                                        depth_mm=(300.0, 900.0)) for b, i in enumerate(idx)]
      dv = {}
      for key in ('obj', 'frag', 'loc'):
        off = np.concatenate([sc[key][0] for sc in scenes])
        val = np.concatenate([sc[key][1].reshape(len(sc[key][0]), -1) for sc in scenes])
        dv[key] = (torch.from_numpy(off).cuda(),
                   torch.from_numpy(np.ascontiguousarray(val)).cuda(), int(val.shape[1]))
      self.plants.append(dv)
    # dry run: the row counts of batch 0's slots decide the cap
    plain.process_batch(self.images[0], self.Ks, TARGETS[0], seed=SEED, after_net=self.planter(0))
    self.totals = sorted(int(t) for t in plain.last_totals[:, 1])
    self.K = self.totals[-2]                   # the largest slot is cut, the others are not

  def pipe(self, **kw):
    from epos_amd import pipeline
    return pipeline.EposPipeline(self.ckpt, B, H, W_, O, F, self.store, capacity=1 << 16, **kw)

  def planter(self, j):
    from epos_amd import _lib, weights
    dv = self.plants[j]

    def plant(p):
      st = ctypes.c_void_p(p.stream.cuda_stream)
      for key, name in (('obj', weights.PRED_OBJ_CONF), ('frag', weights.PRED_FRAG_CONF),
                        ('loc', weights.PRED_FRAG_LOC)):
        off, val, width = dv[key]
        _lib.check(self.lib.epos_scatter_blocks_f32(
            ctypes.c_void_p(p.net.logits[name].data_ptr()), ctypes.c_void_p(off.data_ptr()),
            ctypes.c_void_p(val.data_ptr()), off.numel(), width, st), 'scatter_blocks')
    return plant

  def fused(self, pipe, j):
    return pipe.process_batch(
        self.images[j], self.Ks, TARGETS[j], image_ids=[f.im_id for f in self.frames[j]],
        scene_ids=[f.scene_id for f in self.frames[j]], seed=SEED, after_net=self.planter(j))[0]

  def by_operators(self, pipe, j, prosac, K, method):
    """infer.process_by_operators on the head tensors `pipe` holds after its step (planted
    values included), with the args of the matching command line."""
    import infer
    from epos_amd import fitting
    argv = ['--model', 'm', '--seed', str(SEED), '--use_prosac', str(bool(prosac)),
            '--fitting_method', method]
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
  return World()


def same_poses(a, b):
  assert len(a) == len(b)
  for p, q in zip(a, b):
    assert (p['scene_id'], p['im_id'], p['obj_id']) == (q['scene_id'], q['im_id'], q['obj_id'])
    assert p['score'] == q['score']
    assert np.asarray(p['R']).tobytes() == np.ascontiguousarray(q['R']).tobytes()
    assert np.asarray(p['t']).tobytes() == np.ascontiguousarray(q['t']).tobytes()


def test_cap_splits_the_slots(world):
  """Conditions of the comparisons below: with the cap chosen from the dry run at least one
  slot has more rows than the cap and at least one has between 6 rows and the cap."""
  assert any(n > world.K for n in world.totals)
  assert any(6 <= n <= world.K for n in world.totals)


@pytest.mark.parametrize('prosac,capped,method', [
    (1, True, 'progressive_x'), (1, False, 'progressive_x'), (0, True, 'progressive_x'),
    (1, True, 'opencv_ransac')])
def test_fused_order_equals_operator_path(world, prosac, capped, method):
  from epos_amd import fitting
  K = world.K if capped else None
  pipe = world.pipe(fit_params=fitting.fit_params(use_prosac=prosac), max_correspondences=K,
                    fitting_method=method)
  assert pipe.order is not None
  got = world.fused(pipe, 0)
  exp = world.by_operators(pipe, 0, prosac, K, method)
  assert len(got) >= 1
  same_poses(got, exp)
  check_ordered_buffers(pipe, K, prosac)


def check_ordered_buffers(pipe, K, prosac):
  """What the stage left behind after the step, against the numpy restatement computed from
  the extractor's own buffers (real px_id, real masks): bit for bit."""
  from tests.helpers import order_ref
  S, ex, od = pipe.corr.S, pipe.corr, pipe.order
  host = lambda t: t.cpu().numpy()      # noqa: E731
  slot_base = host(ex.slot_base)[:S + 1]
  n = int(slot_base[-1])
  ref = order_ref.order_stage(host(ex.conf)[:n], host(ex.coord_2d)[:n], host(ex.coord_3d)[:n],
                              slot_base, ex.capacity, K, prosac)
  m = int(ref['slot_base_out'][-1])
  assert m > 0 and ref['applied'].any()
  assert np.array_equal(host(od.slot_base)[:S + 1], ref['slot_base_out'])
  for name in ('src_row', 'yorder', 'ypos'):
    assert np.array_equal(host(getattr(od, name))[:m], ref[name]), name
  for name in ('coord_2d', 'coord_3d'):
    assert host(getattr(od, name))[:m].tobytes() == ref[name].tobytes(), name
  # the case px_id // W cannot order: some slot's kept rows are NOT in row order
  assert any((np.diff(ref['yorder'][a:b]) < 0).any() for a, b in
             zip(ref['slot_base_out'][:-1], ref['slot_base_out'][1:]))


def test_fused_order_with_two_batches_enqueued(world):
  """queue=2: the second batch is enqueued while the first still runs on the same ordered
  buffers (stream order keeps them apart)."""
  from epos_amd import fitting
  fit = fitting.fit_params(use_prosac=1)
  one = world.pipe(fit_params=fit, max_correspondences=world.K)
  exp = []
  for j in range(2):
    exp.append(world.fused(one, j))
    same_poses(exp[j], world.by_operators(one, j, 1, world.K, 'progressive_x'))
  two = world.pipe(fit_params=fit, max_correspondences=world.K, queue=2)
  for j in range(2):
    two.launch(world.images[j], world.Ks, TARGETS[j],
               image_ids=[f.im_id for f in world.frames[j]],
               scene_ids=[f.scene_id for f in world.frames[j]], seed=SEED,
               after_net=world.planter(j))
  got = [two.collect()[0] for _ in range(2)]
  assert sum(len(g) for g in got) >= 2
  for j in range(2):
    same_poses(got[j], exp[j])


def test_plain_pipeline_has_no_ordering_stage(world):
  plain = world.pipe()
  assert plain.order is None and plain.max_correspondences is None


def test_infer_cli_orders_on_the_device_by_default(tmp_path, gpu_children):
  """--use_prosac --max_correspondences through the fused pipeline (more than one step in
  flight) writes the rows of the operator-path run (--order_on_device false)."""
  rows, plans = {}, {}
  for on_device in ('true', 'false'):
    d = tmp_path / on_device
    (d / 'toy').mkdir(parents=True)
    (d / 'toy' / 'params.yml').write_text('infer_crop_size: "128,96"\n')
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, 'infer.py'), '--model=toy', '--synthetic', '2',
         '--num_objs', '3', '--use_prosac', 'true', '--max_correspondences', '200',
         '--order_on_device', on_device],
        env=dict(os.environ, TF_MODELS_PATH=str(d)), capture_output=True, text=True,
        timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    txt = (d / 'toy' / 'infer' / 'estimated-poses.csv').read_text().strip().split('\n')
    rows[on_device] = [','.join(r.split(',')[:-1]) for r in txt]
    plans[on_device] = [l for l in out.stdout.split('\n') if l.startswith('plan: ') and
                        'step(s) in flight' in l][0]
  assert rows['true'] == rows['false']
  assert len(rows['true']) >= 2                    # the header and at least one pose
  steps = lambda line: int(line.split(' step(s) in flight')[0].split()[-1])     # noqa: E731
  assert steps(plans['true']) > 1
  assert steps(plans['false']) == 1
