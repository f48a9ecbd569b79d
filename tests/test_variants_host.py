"""The backbones beyond xception_65 / resnet_v1_101_beta (xception_41, xception_71,
resnet_v1_50_beta, resnet_v1_50, resnet_v1_101), host side: both readings of the network -- the
HIP plan (dry run) and the test oracle tests/helpers/net_ref_variants.py -- build the graphs the
reference's own code builds (tests/golden/variant_graph_*.json, make_graph_golden_variants.py),
the variable names and shapes match those graphs, the flag check accepts the variants, and a
TensorFlow checkpoint under their names restores. CPU only."""
import filecmp
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from epos_amd import weights
from test_graph_trace import _diff, _load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, 'tests', 'golden')
GOLDEN = sorted(glob.glob(os.path.join(GOLDEN_DIR, 'variant_graph_*.json')))
IDS = [os.path.basename(p)[len('variant_graph_'):-5] for p in GOLDEN]
NEW = ['xception_41', 'xception_71', 'resnet_v1_50_beta', 'resnet_v1_50', 'resnet_v1_101']


def _ckpt(cfg):
  return weights.random_init(cfg['model_variant'], num_objs=cfg['num_objs'],
                             num_frags=cfg['num_frags'], seed=0)


def test_fixtures_cover_the_new_variants():
  cfgs = [_load(p)['config'] for p in GOLDEN]
  assert {c['model_variant'] for c in cfgs} == set(NEW)
  assert all((c['width'], c['height'], c['num_objs'], c['num_frags']) == (640, 480, 21, 64)
             for c in cfgs)
  assert any(c['multi_grid'] == [1, 2, 4] and 'resnet' in c['model_variant'] for c in cfgs)
  for p in GOLDEN:
    assert os.path.getsize(p) < 1 << 20, p


@pytest.mark.parametrize('path', GOLDEN, ids=IDS)
def test_root_and_preprocessing_as_the_reference_builds_them(path):
  g = _load(path)
  v = g['config']['model_variant']
  first = g['layers'][0]
  if v in ('resnet_v1_50', 'resnet_v1_101'):
    # one 7x7 stride-2 conv2d_same on the mean-subtracted image, padded after preprocessing
    assert first['scope'] == v + '/conv1'
    assert (first['kernel'], first['stride'], first['padding']) == ([7, 7], 2, 'VALID')
    assert first['input'] == 'pad(submean(input),3,3)'
  else:
    assert first['kernel'] == [3, 3] and first['input'] == 'pad(preprocess(input),1,1)'
  tap = [l for l in g['layers'] if l['scope'] == 'decoder/feature_projection0'][0]['input']
  want = {'xception_71': 'entry_flow/block3/unit_1/xception_module/separable_conv2_pointwise',
          'xception_41': 'entry_flow/block2/unit_1/xception_module/separable_conv2_pointwise'
          }.get(v, 'block1/unit_2/bottleneck_v1/conv3')
  assert tap.endswith('/' + want), tap


@pytest.mark.parametrize('path', GOLDEN, ids=IDS)
def test_hip_plan_builds_the_reference_graph(path):
  from epos_amd import net
  g = _load(path)
  cfg = g['config']
  plan = net.EposNet(_ckpt(cfg), 1, cfg['height'], cfg['width'], cfg['num_objs'],
                     cfg['num_frags'], model_variant=cfg['model_variant'],
                     multi_grid=cfg['multi_grid'], atrous_rates=tuple(cfg['atrous_rates']),
                     dry_run=True)
  d = _diff(g['layers'], plan.trace_layers)
  assert not d, d[:5]
  assert len(plan.trace_layers) == len(g['layers'])
  assert plan.trace_outputs == g['outputs']
  launched = '+'.join(n for n, _ in plan.ops)
  for l in g['layers']:
    assert l['scope'] in launched, l['scope']
  if cfg['model_variant'] in ('resnet_v1_50', 'resnet_v1_101'):
    assert plan.ops[1][0] == cfg['model_variant'] + '/conv1/im2col'
    assert plan.op_kind[plan.ops[1][0]] == 'im2col'


@pytest.mark.parametrize('path', GOLDEN, ids=IDS)
def test_oracle_helper_builds_the_reference_graph(path):
  from oracle import net_ref
  from helpers import net_ref_variants as nv
  g = _load(path)
  cfg = g['config']
  img = np.zeros((1, cfg['height'], cfg['width'], 3), np.float32)
  net_ref.DEVICE = 'meta'
  try:
    with net_ref.trace() as tr:
      nv.predict(img, _ckpt(cfg), num_objs=cfg['num_objs'], num_frags=cfg['num_frags'],
                 model_variant=cfg['model_variant'], multi_grid=cfg['multi_grid'],
                 atrous_rates=tuple(cfg['atrous_rates']),
                 encoder_output_stride=cfg['encoder_output_stride'],
                 decoder_output_stride=tuple(cfg['decoder_output_stride']))
  finally:
    net_ref.DEVICE = None
  assert tr.layers == g['layers'], _diff(g['layers'], tr.layers)[:5]   # same ORDER too
  assert tr.outputs == g['outputs']


@pytest.mark.parametrize('path', GOLDEN, ids=IDS)
def test_variable_specs_match_the_reference_graph(path):
  """Every parametrised layer of the graph is a variable of variable_specs with its shape,
  and nothing else is; BN epsilon 1e-5 for the resnets, 1e-3 for the xceptions."""
  g = _load(path)
  cfg = g['config']
  specs = {s[1]: (s[0], tuple(s[2])) for s in weights.variable_specs(
      cfg['model_variant'], cfg['num_objs'], cfg['num_frags'])}
  assert set(specs) == {l['scope'] for l in g['layers']}
  eps = 1e-5 if 'resnet' in cfg['model_variant'] else 1e-3
  scope = {'resnet_v1_50_beta': 'resnet_v1_50'}.get(cfg['model_variant'],
                                                    cfg['model_variant'])
  for l in g['layers']:
    kind, shape = specs[l['scope']]
    kh, kw = l['kernel']
    if l['op'] == 'depthwise_conv2d':
      assert (kind, shape) == ('dw', (kh, kw, l['cin'], 1)), l['scope']
    else:
      assert kind in ('conv', 'logits') and shape == (kh, kw, l['cin'], l['cout']), l['scope']
    if l['scope'].startswith(scope + '/'):
      assert l['bn_eps'] == eps, l['scope']


def test_unknown_variants_still_raise():
  from epos_amd import net
  for bad in ('mobilenet_v2', 'nas_pnasnet', 'xception_99'):
    with pytest.raises(ValueError):
      weights.variable_specs(bad)
    with pytest.raises(ValueError):
      net.EposNet({}, 1, 64, 64, 1, model_variant=bad, dry_run=True)


def test_check_supported_flags_accepts_the_variants():
  import infer
  from epos_amd import cli
  for v in NEW + ['xception_65', 'resnet_v1_101_beta']:
    args = infer.build_parser().parse_args(['--model', 'm', '--model_variant', v])
    cli.check_supported_flags(args)
  args = infer.build_parser().parse_args(['--model', 'm', '--model_variant', 'mobilenet_v2'])
  with pytest.raises(NotImplementedError):
    cli.check_supported_flags(args)


@pytest.mark.parametrize('variant', ['resnet_v1_50', 'xception_71', 'resnet_v1_50_beta'])
def test_tf_checkpoint_restores_by_name(tmp_path, variant):
  from epos_amd import tf_checkpoint as tc
  ckpt = weights.random_init(variant, num_objs=2, seed=1, randomize_bn=True)
  if variant == 'resnet_v1_50':
    assert ckpt['resnet_v1_50/conv1/weights'].shape == (7, 7, 3, 64)
  if variant == 'resnet_v1_50_beta':
    assert 'resnet_v1_50/conv1_1/weights' in ckpt
  full = dict(ckpt)
  full['global_step'] = np.asarray(100, np.int64)
  full[sorted(ckpt)[0] + '/Momentum'] = np.zeros_like(ckpt[sorted(ckpt)[0]])
  prefix = str(tmp_path / 'model.ckpt-100')
  tc.write_checkpoint(prefix, full)
  back = tc.to_epos_checkpoint(tc.load_checkpoint(prefix))
  assert set(back) == set(ckpt)
  for k in ckpt:
    assert np.array_equal(back[k], ckpt[k]), k
  from epos_amd import net
  net.EposNet(back, 1, 96, 128, 2, model_variant=variant, dry_run=True)


def test_generator_reproduces_the_fixtures(tmp_path):
  """make_graph_golden_variants.py, run against the reference, writes the committed bytes."""
  sys.path.insert(0, GOLDEN_DIR)
  import make_graph_golden as M
  if not os.path.isdir(os.path.join(M.REFERENCE, 'epos_lib')):
    pytest.skip('the reference checkout the generators read is not on this machine')
  r = subprocess.run([sys.executable, os.path.join(GOLDEN_DIR, 'make_graph_golden_variants.py'),
                      '--out', str(tmp_path)], capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stdout + r.stderr
  made = sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / '*.json')))
  assert made == [os.path.basename(p) for p in GOLDEN]
  for name in made:
    assert filecmp.cmp(str(tmp_path / name), os.path.join(GOLDEN_DIR, name), shallow=False), name
