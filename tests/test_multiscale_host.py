"""CPU tests of multi-scale inference (image_pyramid + merge_method, model.py:515-626): the
sizes of every scale's plan and of the merged heads, argument validation, infer.py's flag
handling, and the structure of the dry-run MultiScaleNet against the oracle's graph at every
scale."""
import os

import numpy as np
import pytest

from helpers import multiscale_ref as msr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, W, pyramid) -> per-scale input sizes, their stride-4 sizes, merged (Lh, Lw); by hand from
# scale_dimension (model.py:100-114): int((d - 1) * s + 1); inputs model.py:569-573, merged
# size at max(1, max(P)) / 4 (model.py:559-562)
SIZES = [
    (480, 640, [0.75, 1.0, 1.25],
     [(360, 480), (480, 640), (599, 799)], [(90, 120), (120, 160), (150, 200)], (150, 200)),
    (480, 640, [0.75, 1.0],
     [(360, 480), (480, 640)], [(90, 120), (120, 160)], (120, 160)),
    (540, 720, [0.75, 1.0, 1.25],
     [(405, 540), (540, 720), (674, 899)], [(102, 135), (135, 180), (169, 225)], (169, 225)),
    (64, 96, [0.5, 1.0, 1.25],
     [(32, 48), (64, 96), (79, 119)], [(8, 12), (16, 24), (20, 30)], (20, 30)),
    (64, 96, [0.5], [(32, 48)], [(8, 12)], (16, 24)),
    (64, 96, [0.5, 0.75], [(32, 48), (48, 72)], [(8, 12), (12, 18)], (16, 24)),
    (480, 640, [0.5, 0.75, 1.0, 1.25, 1.5, 1.75],
     [(240, 320), (360, 480), (480, 640), (599, 799), (719, 959), (839, 1119)],
     [(60, 80), (90, 120), (120, 160), (150, 200), (180, 240), (210, 280)], (210, 280)),
]


@pytest.mark.parametrize('h,w,pyr,inputs,logits,merged', SIZES)
def test_scale_sizes_by_hand(h, w, pyr, inputs, logits, merged):
  from epos_amd import multiscale as ms
  assert ms.scale_sizes(h, w, pyr) == inputs
  assert ms.merged_size(h, w, pyr) == merged == msr.merged_size(h, w, pyr)
  assert [(ms._net.scale_dimension(a, 0.25), ms._net.scale_dimension(b, 0.25))
          for a, b in inputs] == logits


def test_dry_run_plan_sizes_and_launch_order():
  from epos_amd import multiscale as ms, weights
  ckpt = weights.random_init(num_objs=2, num_frags=8, seed=0)
  n = ms.MultiScaleNet(ckpt, 2, 64, 96, 2, 8, image_pyramid=[0.5, 1.0, 1.25],
                       merge_method='avg', dry_run=True)
  assert (n.out_h, n.out_w, n.B, n.H, n.W) == (20, 30, 2, 64, 96)
  # a scale != 1 decodes at crop_size [h_s, w_s] read as [w, h] (model.py:355-356,572,581)
  assert [(p.H, p.W, p.out_h, p.out_w) for p in n.nets] == [
      (32, 48, 12, 8), (64, 96, 16, 24), (79, 119, 30, 20)]
  assert n.images is n.nets[1].images             # the 1.0 plan's input buffer is the image
  assert [name for name, _ in n.ops] == [
      'scale_0.5/resize_input', 'scale_0.5/plan', 'scale_1/plan',
      'scale_1.25/resize_input', 'scale_1.25/plan',
      'merge/pred_frag_conf', 'merge/pred_frag_loc', 'merge/pred_obj_conf']
  assert {k: tuple(v.shape) for k, v in n.logits.items()} == {
      'pred_obj_conf': (2, 20, 30, 3), 'pred_frag_conf': (2, 20, 30, 16),
      'pred_frag_loc': (2, 20, 30, 48)}
  assert n.flops == sum(p.flops for p in n.nets) > 0
  ch = 3 + 16 + 48
  src = sum(2 * p.out_h * p.out_w for p in n.nets) * ch
  img = 2 * 64 * 96 * 3 * 2 + 2 * 3 * (32 * 48 + 79 * 119)
  assert n.merge_bytes == 4 * (src + 2 * 20 * 30 * ch + img)
  # no 1.0 plan: a full-size image buffer of its own
  n2 = ms.MultiScaleNet(ckpt, 1, 64, 96, 2, 8, image_pyramid=[0.5, 0.75], dry_run=True)
  assert tuple(n2.images.shape) == (1, 64, 96, 3)
  assert all(n2.images is not p.images for p in n2.nets)
  assert (n2.out_h, n2.out_w) == (16, 24)


@pytest.mark.parametrize('bad', [[], [0.0, 1.0], [-0.5], [1.0] * 9, [float('nan')],
                                 [float('inf'), 1.0], 'abc'])
def test_invalid_pyramid_raises(bad):
  from epos_amd import model, multiscale as ms
  with pytest.raises(ValueError):
    ms.normalize_pyramid(bad)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(1, 8))
  with pytest.raises(ValueError):
    model.get_net({}, 1, 64, 64, 1, 8, mo, image_pyramid=bad)


def test_single_scale_stays_on_eposnet_and_merge_method_is_checked():
  from epos_amd import model, multiscale as ms
  assert ms.normalize_pyramid(None) is None
  assert ms.normalize_pyramid([1.0]) is None and ms.normalize_pyramid((1,)) is None
  assert ms.normalize_pyramid([1.0] * 8) == [1.0] * 8
  assert ms.normalize_pyramid((0.5, 1)) == [0.5, 1.0]
  mo = model.ModelOptions(model.get_outputs_to_num_channels(1, 8))
  assert mo.merge_method == 'max' and len(mo) == 13
  assert model.ModelOptions({}, merge_method='avg').merge_method == 'avg'
  for bad in ['mean', 'sum', None, 'MAX']:
    with pytest.raises(ValueError):
      model.ModelOptions({}, merge_method=bad)
    with pytest.raises(ValueError):
      ms.MultiScaleNet({}, 1, 64, 64, 1, 8, image_pyramid=[0.5, 1.0], merge_method=bad,
                       dry_run=True)


def test_merge_statement_small_cases():
  """The numpy statement itself: identity at the same size, corners kept, mean / max."""
  rng = np.random.RandomState(0)
  x = rng.standard_normal((2, 5, 7, 3)).astype(np.float32)
  assert np.array_equal(msr.resize(x, 5, 7), x)
  y = msr.resize(x, 9, 13)
  assert y.dtype == np.float32
  for yy, xx in [(0, 0), (8, 12), (0, 12), (8, 0)]:
    assert np.array_equal(y[:, yy, xx], x[:, yy * 4 // 8, xx * 6 // 12])
  assert np.array_equal(msr.resize(x, 1, 1), x[:, :1, :1])
  a, b = x, rng.standard_normal(x.shape).astype(np.float32)
  assert np.array_equal(msr.resize_merge([a, b], 5, 7, 'max'), np.maximum(a, b))
  assert np.array_equal(msr.resize_merge([a, b], 5, 7, 'avg'), (a + b) / np.float32(2))


def _args(extra):
  import infer
  return infer.build_parser().parse_args(['--model', 'm'] + extra)


def test_infer_flags_accept_a_pyramid_only_when_asked():
  from epos_amd import cli
  for extra in (['--image_pyramid', '0.75,1.0,1.25'],
                ['--image_pyramid', '0.5', '--merge_method', 'avg']):
    with pytest.raises(NotImplementedError):
      cli.check_supported_flags(_args(extra))
    cli.check_supported_flags(_args(extra + ['--multi_scale_inference', 'true']))
  assert _args([]).multi_scale_inference is False
  cli.check_supported_flags(_args(['--image_pyramid', '1.0']))
  for extra in (['--image_pyramid', '0.5,1.0', '--merge_method', 'median'],
                ['--image_pyramid', '0,1.0'],
                ['--image_pyramid', ','.join(['1.0'] * 9)]):
    with pytest.raises(ValueError):
      cli.check_supported_flags(_args(extra + ['--multi_scale_inference', 'true']))


def test_infer_params_yml_pyramid_with_the_flag(tmp_path):
  from epos_amd import cli
  args = _args(['--multi_scale_inference', 'true'])
  p = tmp_path / 'params.yml'
  p.write_text('image_pyramid: [0.5, 1.0]\nmerge_method: avg\n')
  cli.update_flags(args, str(p))
  cli.check_supported_flags(args)
  assert cli.as_list(args.image_pyramid, float) == [0.5, 1.0]


def test_sparse_heads_with_a_pyramid():
  """--sparse_heads auto resolves to dense with a pyramid, true raises."""
  import infer
  loc = ['--task_type', 'localization']
  assert infer.resolve_sparse_heads(_args(loc), False, None) is True
  assert infer.resolve_sparse_heads(_args(loc), False, [0.5, 1.0]) is False
  assert infer.resolve_sparse_heads(_args(loc + ['--sparse_heads', 'false']), False,
                                    [0.5, 1.0]) is False
  with pytest.raises(ValueError):
    infer.resolve_sparse_heads(_args(loc + ['--sparse_heads', 'true']), False, [0.5, 1.0])
  assert infer.resolve_sparse_heads(_args(loc + ['--sparse_heads', 'true']), False, None)


def test_pipeline_refuses_sparse_heads_with_a_pyramid():
  from epos_amd import pipeline
  with pytest.raises(ValueError):
    pipeline.EposPipeline({}, 1, 64, 64, 1, 8, None, image_pyramid=[0.5, 1.0],
                          sparse_heads=True)
  with pytest.raises(ValueError):
    pipeline.EposPipeline({}, 1, 64, 64, 1, 8, None, image_pyramid=[0.5, 1.0],
                          merge_method='median')


def test_repeated_scales_collapse_as_the_reference_keys_them():
  """multi_scale_logits keys the per-scale logits by 'logits_%.2f' % scale (model.py:603-606):
  scales that print alike are one merge entry, holding the LAST of them at the FIRST one's
  position; the merged size follows the pyramid as given (model.py:559-562)."""
  from epos_amd import multiscale as ms, weights
  assert ms.merged_scales([1.0, 1.0]) == [1.0]
  assert ms.merged_scales([0.5, 1.0, 1.0]) == [0.5, 1.0]
  assert ms.merged_scales([1.0, 0.5, 1.004, 0.501]) == [1.004, 0.501]
  assert msr.merged_scales([1.0, 0.5, 1.004, 0.501]) == [1.004, 0.501]
  ckpt = weights.random_init(num_objs=2, num_frags=8, seed=0)
  n = ms.MultiScaleNet(ckpt, 1, 64, 96, 2, 8, image_pyramid=[1.0, 1.0], dry_run=True)
  assert n.scales == [1.0] and len(n.nets) == 1 and n.images is n.nets[0].images
  assert [name for name, _ in n.ops] == [
      'scale_1/plan', 'merge/pred_frag_conf', 'merge/pred_frag_loc', 'merge/pred_obj_conf']
  n = ms.MultiScaleNet(ckpt, 1, 64, 96, 2, 8, image_pyramid=[1.0, 0.5, 1.0, 1.004],
                       dry_run=True)
  assert n.scales == [1.004, 0.5] and n.trace['merge']['pred_obj_conf']['keys'] == [
      'logits_1.00', 'logits_0.50']
  # 1.004 is a resized 64x96 input whose decoder reads crop_size [64, 96] as [w, h]
  assert [(p.H, p.W, p.out_h, p.out_w) for p in n.nets] == [(64, 96, 24, 16), (32, 48, 12, 8)]
  assert (n.out_h, n.out_w) == (16, 24)
  assert 'scale_1.004/resize_input' in [name for name, _ in n.ops]


def test_dry_run_structure_matches_the_reference_fixture():
  """C2 (640x480, 21 objects) with [0.75, 1.0, 1.25], max: the dry-run plan against the graph
  the reference's own multi_scale_logits builds (tests/golden/make_graph_golden_pyramid.py):
  per scale the image the network sees and every layer (scope, shapes, input expression),
  every logits resize, the merge entries and the merged size."""
  import json
  from epos_amd import multiscale as ms, weights
  with open(os.path.join(ROOT, 'tests', 'golden',
                         'pyramid_graph_c2_xception65_640x480_o21.json')) as f:
    g = json.load(f)
  cfg = g['config']
  O, F = cfg['num_objs'], cfg['num_frags']
  ckpt = weights.random_init(num_objs=O, num_frags=F, seed=0)
  n = ms.MultiScaleNet(ckpt, 1, cfg['height'], cfg['width'], O, F,
                       image_pyramid=cfg['image_pyramid'], merge_method=cfg['merge_method'],
                       dry_run=True)
  tr = n.trace
  assert len(tr['per_scale']) == len(g['per_scale'])
  # (the plan records its layers in launch order, the graph in definition order: compared
  # by scope, as tests/test_graph_trace.py does)
  by_scope = lambda layers: {l['scope']: l for l in layers}
  for got, ref in zip(tr['per_scale'], g['per_scale']):
    assert got['scale'] == ref['scale']
    assert got['input_hw'] == ref['input_hw'] and got['input_expr'] == ref['input_expr']
    assert len(got['layers']) == len(ref['layers']), got['scale']
    # a plan's own input is the scale's image: 'input' there is ref['input_expr'] here, and
    # the recorder spells out (2/255) * x - 1 (feature.py:171-174) on anything but 'input'
    x = ref['input_expr']
    pre_ref = 'sub(mul(%s,%.9g),1)' % (x, 2.0 / 255.0)
    canon = lambda l, a, b: dict(l, input=l['input'].replace(a, b))
    want = by_scope([canon(l, pre_ref, 'preprocess(%s)' % x) for l in ref['layers']])
    have = by_scope([canon(l, 'preprocess(input)', 'preprocess(%s)' % x)
                     for l in got['layers']])
    assert have == want, got['scale']
  assert tr['logits_resize'] == g['logits_resize']
  for name, m in g['merge'].items():
    assert tr['merge'][name]['keys'] == m['keys'], name
    assert tr['merge'][name]['target'] == m['shape'][1:3], name
    assert tr['merge'][name]['channels'] == m['shape'][3], name
    assert m['expr'].startswith('reduce_%s(stack(' % cfg['merge_method']), name
    assert m['expr'].count('expand(') == len(tr['merge'][name]['sources']), name
  assert tr['merged_hw'] == g['outputs']['pred_obj_conf']['shape'][1:3]
