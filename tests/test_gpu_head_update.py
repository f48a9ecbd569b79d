"""The weight update on the device: epos_pack_weights_device_f32 against the three host packers
byte for byte, its refusals (all or nothing), EposNet.set_weights against a freshly built
net (eager, captured graphs, sparse heads) and trainer.train_step against its parts."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import loss_cases, pack_cases   # noqa: E402
from tests.helpers.loss_device import KEYS as HEADS, gt_tensors   # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUTS = ('plain', 'split', 'h2', 'bias')


@pytest.fixture(scope='module')
def lib():
  from epos_amd import _lib
  return _lib.load()


def assert_packed(lib, probs, status, dsts, tag):
  assert status.tolist() == [0] * len(probs), (tag, status)
  for i, (prob, d) in enumerate(zip(probs, dsts)):
    ref = pack_cases.host_pack(lib, *prob)
    assert ref['h2'] is not None, (tag, i)
    for k in LAYOUTS:
      assert d[k].size == ref[k].size, (tag, i, k, d[k].size, ref[k].size)
      diff = np.nonzero(d[k] != ref[k])[0]
      assert diff.size == 0, (tag, i, prob[0].shape, prob[2:], k, diff[:8],
                              d[k][diff[:8]], ref[k][diff[:8]])


# ------------------------------------------------------------------ packer ---
@pytest.mark.parametrize('kind', pack_cases.VALUE_SETS)
def test_packer_equals_the_host_packers(lib, kind):
  probs = pack_cases.problems(kind, seed=100)
  # the padding is written: K = 20 pads the plain layout to 32 rows and the others to 32 too,
  # N = 129 leaves 127 padding columns -- and every destination starts as 0xA5 bytes
  for i, prob in enumerate(probs):                 # alone
    status, dsts = pack_cases.device_pack(lib, [prob])
    assert_packed(lib, [prob], status, dsts, (kind, 'alone', i))
  status, dsts = pack_cases.device_pack(lib, probs)   # one grouped call of different sizes
  assert_packed(lib, probs, status, dsts, (kind, 'grouped'))


def test_value_sets_hold_what_they_claim(lib):
  w, _ = pack_cases.matrix('subnormal', 8, 5, 0)
  assert (np.abs(w[w != 0]) < np.finfo(np.float32).tiny).sum() == 1
  w, _ = pack_cases.matrix('tiny', 8, 5, 0)
  assert np.abs(w[1:]).max() < 2.0 ** -27 and (w[0] == 1).all()
  # such weights have fp16-subnormal pieces: hi of 2^-30 * 2^14 = 2^-16 is below 2^-14
  w, _ = pack_cases.matrix('negative_zero', 8, 5, 0)
  assert np.signbit(w[4]).all() and (w[4] == 0).all()
  w, _ = pack_cases.matrix('zero_column', 8, 5, 0)
  assert (w[:, 2] == 0).all()


def test_more_problems_than_one_launch_holds_and_two_runs_same_bytes(lib):
  probs = [p for s in range(6) for p in pack_cases.problems('heavy_tailed', seed=10 * s)][:45]
  assert len(probs) == 45                          # the workload's count: two launches of <= 32
  status, first = pack_cases.device_pack(lib, probs)
  assert_packed(lib, probs, status, first, 'chunks')
  status2, second = pack_cases.device_pack(lib, probs)
  assert status2.tolist() == status.tolist()
  for a, b in zip(first, second):
    for k in LAYOUTS:
      assert a[k].tobytes() == b[k].tobytes(), k


def poisoned(what):
  w, b = pack_cases.matrix('normal', 8, 5, 7)
  if what == 'inf':
    w[3, 2] = np.inf
  elif what == 'nan':
    w[5, 4] = np.nan
  elif what == 'max_2^120':
    w[1, 0] = 2.0 ** 120
  else:
    assert what == 'only_2^-120'
    w[:, 3] = 0.0
    w[6, 3] = 2.0 ** -120
  return w, b, 0, 5


@pytest.mark.parametrize('what', ['inf', 'nan', 'max_2^120', 'only_2^-120'])
@pytest.mark.parametrize('where', [0, 1, 2, 40])
def test_refusals_are_the_host_packers_and_all_or_nothing(lib, what, where):
  good = pack_cases.problems('normal', seed=3)
  probs = [good[2], good[3], good[4]]
  if where == 40:                                  # the refused problem in the second launch
    probs = (good * 6)[:44]
  where = min(where, len(probs))
  bad = poisoned(what)
  probs.insert(where, bad)
  assert pack_cases.host_pack(lib, *bad)['h2'] is None          # the host packer returns 0
  for i, p in enumerate(probs):
    assert (pack_cases.host_pack(lib, *p)['h2'] is None) == (i == where)
  status, dsts = pack_cases.device_pack(lib, probs)
  assert status[where] != 0 and (np.delete(status, where) == 0).all(), status
  for d in dsts:                                   # not one byte of any problem
    for k in LAYOUTS:
      assert (d[k] == pack_cases.FILL).all(), k
  # without the fp16-pair destination nothing is refused: the other layouts are written
  status, dsts = pack_cases.device_pack(lib, probs, want=('plain', 'split', 'bias'))
  assert status.tolist() == [0] * len(probs)
  for i, (p, d) in enumerate(zip(probs, dsts)):
    ref = pack_cases.host_pack(lib, *p)
    assert d['plain'].tobytes() == ref['plain'].tobytes(), i    # a copy: NaN and Inf included
    assert d['bias'].tobytes() == ref['bias'].tobytes(), i
    if i != where or what.endswith('120'):         # the NaN pieces of Inf - Inf: unspecified
      assert d['split'].tobytes() == ref['split'].tobytes(), i


# --------------------------------------------------------------------- net ---
H, W, O, F, B = 96, 128, 3, 64, 2


def six(ckpt):
  from epos_amd import heads_train
  return {n: ckpt[n] for h in HEADS for n in heads_train.variable_names(h)}


def build(ckpt):
  from epos_amd import net
  return net.EposNet(ckpt, B, H, W, O, F, device='cuda:0')


@pytest.fixture(scope='module')
def ckpts():
  """Checkpoint A, and A with the six logits variables of a second random init."""
  from epos_amd import weights
  a = weights.random_init('xception_65', num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  b = weights.random_init('xception_65', num_objs=O, num_frags=F, seed=1, logits_std=0.05)
  ab = dict(a)
  ab.update(six(b))
  return a, ab


@pytest.fixture(scope='module')
def images():
  from epos_amd import synthetic
  return np.stack([synthetic.image(i, H, W) for i in range(B)]).astype(np.float32)


@pytest.fixture(scope='module')
def net_a(ckpts):
  """Built from A and never updated."""
  return build(ckpts[0])


@pytest.fixture(scope='module')
def net_b(ckpts):
  """Built by the host packers from A with the second heads, never updated."""
  return build(ckpts[1])


@pytest.fixture(scope='module')
def net_upd(ckpts, images):
  """Built from A, with both graphs captured before any update; the tests below update it."""
  n = build(ckpts[0])
  n.forward_logits(images, use_graph=True)
  n.forward(images, use_graph=True)
  torch.cuda.synchronize()
  return n


def host(d):
  torch.cuda.synchronize()
  return {k: v.cpu().numpy().copy() for k, v in d.items()}


SLOTS = [(0, 2), (1, 3)]


def sparse_bytes(n, images):
  n.forward_logits(images)
  n.run_sparse_heads(SLOTS, torch.tensor(SLOTS, dtype=torch.int32, device='cuda:0'))
  return host({k: n.logits[k] for k in HEADS})


def all_runs(n, images):
  return {'logits_eager': host(n.forward_logits(images)),
          'logits_graph': host(n.forward_logits(images, use_graph=True)),
          'forward_eager': host(n.forward(images)),
          'forward_graph': host(n.forward(images, use_graph=True)),
          'sparse': sparse_bytes(n, images)}


def assert_same(got, want, tag):
  for run in want:
    for k in want[run]:
      assert got[run][k].tobytes() == want[run][k].tobytes(), (tag, run, k)


@pytest.mark.parametrize('packs', ['built_before', 'built_after'])
def test_set_weights_equals_a_freshly_built_net(ckpts, images, net_a, net_b, net_upd, packs):
  a, ab = ckpts
  graphs = (net_upd._graph, net_upd._graph_logits)
  assert None not in graphs
  net_upd.set_weights(six(a))                 # whatever an earlier test left
  if packs == 'built_before':
    sparse_bytes(net_upd, images)
    assert net_upd._sparse_packs is not None
  else:
    net_upd._sparse_packs = None
  want_a, want_b = all_runs(net_a, images), all_runs(net_b, images)
  assert want_a['logits_eager']['pred_obj_conf'].tobytes() != \
      want_b['logits_eager']['pred_obj_conf'].tobytes()
  status = net_upd.set_weights(
      {k: torch.from_numpy(v).cuda() for k, v in six(ab).items()})
  assert status.dtype == torch.int32 and status.tolist() == [0] * (3 + 2 * O)
  assert_same(all_runs(net_upd, images), want_b, packs)
  assert (net_upd._graph, net_upd._graph_logits) == graphs       # the graphs from before
  # one layer only (numpy arrays, [256, N] weights): the other two heads keep their bytes
  name = 'logits/pred_frag_conf/'
  net_upd.set_weights({name + 'weights': a[name + 'weights'].reshape(256, -1),
                       name + 'biases': a[name + 'biases']})
  got = all_runs(net_upd, images)
  for run in ('logits_eager', 'logits_graph', 'sparse'):
    assert got[run]['pred_frag_conf'].tobytes() == want_a[run]['pred_frag_conf'].tobytes(), run
    for k in ('pred_obj_conf', 'pred_frag_loc'):
      assert got[run][k].tobytes() == want_b[run][k].tobytes(), (run, k)


def test_refusal_through_the_net_and_argument_checks(ckpts, images, net_upd):
  from epos_amd._lib import EposError
  a, ab = ckpts
  net_upd.set_weights(six(a))
  before = host(net_upd.forward_logits(images))
  bad = six(ab)
  w = bad['logits/pred_frag_loc/weights'].copy()
  w[0, 0, 17, 100] = np.nan
  bad['logits/pred_frag_loc/weights'] = w
  with pytest.raises(EposError, match=r'refused logits/pred_frag_loc.*previous weights'):
    net_upd.set_weights(bad)
  after = host(net_upd.forward_logits(images))
  for k in before:
    assert after[k].tobytes() == before[k].tobytes(), k
  status = net_upd.set_weights(bad, check=False)
  # sorted layers: frag_conf, frag_loc, obj_conf; then 3 + 3 sparse packs: column 100 of
  # pred_frag_loc lies in the pack of object 1
  assert torch.nonzero(status).flatten().tolist() == [1, 6]
  good = {k: torch.from_numpy(v).cuda() for k, v in six(a).items()}
  name = 'logits/pred_obj_conf/weights'
  for variables, exc in ((dict(good, **{name: good[name].double()}), TypeError),
                         (dict(good, **{name: good[name].cpu()}), ValueError),
                         (dict(good, **{name: good[name][..., :3]}), ValueError),
                         (dict(good, **{'logits/other/weights': good[name]}), ValueError),
                         ({name: good[name]}, ValueError)):
    with pytest.raises(exc):
      net_upd.set_weights(variables)


# -------------------------------------------------------------- train_step ---
def gt_fields(h, w, seed):
  return gt_tensors(loss_cases.make_case(B, h * w, O, F, seed=seed), h, w)


def test_train_step_equals_its_parts(ckpts, images, net_a):
  from epos_amd import trainer
  a = ckpts[0]
  lr, kw = 1e-3, dict(momentum=0.9, weight_decay=4e-5)
  gt = gt_fields(net_a.out_h, net_a.out_w, seed=41)
  # what the parent commit allows: gradients and the step on one net, then a NEW net built by
  # the host packers from the optimiser's state for the second step
  ref_opt = trainer.Optimizer(a, lr=lr, **kw)
  ref_values = []
  net_a.forward_logits(images)
  values, bad, grads = trainer.net_grads(net_a, gt, ref_opt.params)
  ref_values.append(values.cpu().numpy().copy())
  ref_opt.step(grads, lr)
  state = ref_opt.state()
  second = dict(a)
  second.update({k: v for k, v in state.items() if not k.endswith('/Momentum')})
  net2 = build(second)
  net2.forward_logits(images)
  values, bad, grads = trainer.net_grads(net2, gt, ref_opt.params)
  ref_values.append(values.cpu().numpy().copy())
  ref_opt.step(grads, lr)
  ref_state = ref_opt.state()
  # two train_steps on ONE net
  trainee = build(a)
  opt = trainer.Optimizer(a, lr=lr, **kw)
  got_values = []
  for _ in range(2):
    values, bad, status = trainer.train_step(trainee, images, gt, opt, lr)
    got_values.append(values.cpu().numpy().copy())
    assert bad.tolist() == [0] * B and status.tolist() == [0] * (3 + 2 * O)
  for step in range(2):
    assert got_values[step].tobytes() == ref_values[step].tobytes(), (
        step, got_values[step], ref_values[step])
  assert np.isfinite(got_values).all()
  assert got_values[1][3] != got_values[0][3]      # the update reached the net
  got_state = opt.state()
  assert sorted(got_state) == sorted(ref_state) and len(got_state) == 12
  for k in ref_state:
    assert got_state[k].tobytes() == ref_state[k].tobytes(), k
  # resuming: an optimiser restored from that state continues with the same bytes
  resumed = trainer.Optimizer(got_state, lr=lr, **kw)
  for k in got_state:
    t = resumed.accums[k[:-9]] if k.endswith('/Momentum') else resumed.params[k]
    assert t.cpu().numpy().tobytes() == got_state[k].tobytes(), k
