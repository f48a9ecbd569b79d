#!/usr/bin/env python
"""EPOS evaluation on MI355X -- drop-in for ``scripts/eval.py`` of thodan/epos.

    python eval.py --model=<model_name> [flags]                        (eval.py:13-14)

Same contract as the reference script:
  * env TF_DATA_PATH / TF_MODELS_PATH / BOP_PATH; <TF_MODELS_PATH>/<model>/params.yml overrides
    flag defaults; weights from <model>/train/ as ``infer.py`` finds them;
  * annotated frames from ``--eval_tfrecord_names a,b`` (<TF_DATA_PATH>/<name>.tfrecord), every
    annotated instance of the dataset's objects, no visibility filter (eval.py:113-131);
  * results in <model>/eval/: cm_<global_step>.txt, a TensorBoard event file with
    eval/obj_cls_miou_all and eval/obj_cls_miou_fg (eval_utils.py:78-115), and
    last_evaluation.json = {time, checkpoint_path}; a run is skipped when that checkpoint has
    been evaluated or fewer than --eval_interval_secs have passed (eval.py:74-92, 235-241).

What this build adds: metrics_<global_step>.json (the numbers of the table and the scalars),
and fragment counts -- eval/frag_acc and eval/frag_acc_seg, which the reference does not define
(its hook lists the fragment tensors commented out; DESIGN.md, "Evaluation");
``--eval_frag_labels false`` leaves them out. ``--batch_size`` images go through the network at
once (the reference is fixed at 1 because its ground-truth tensors are ragged; here they are
maps). ``--frames <dir>`` (frames.json with gt_poses) and ``--synthetic N`` work as in
``infer.py``, so that the script runs without a dataset.

The ground-truth maps are rendered on the device from the object meshes (epos_amd/render.py),
so the run needs --dataset and $BOP_PATH with the 'eval' models. Only the network runs, with
dense heads; each batch's forward pass, ground-truth maps and table update are enqueued on one
stream and nothing is downloaded before the tables are written.
"""
import argparse
import collections
import json
import os
import sys
import time

import numpy as np     # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import infer           # noqa: E402
from epos_amd import eval_utils   # noqa: E402

# flags of infer.py's parser this script shares: the model flags of epos_lib/common.py and this
# build's input / precision options
_SHARED_FLAGS = (
    'model', 'master', 'checkpoint_name', 'dataset', 'num_frags', 'model_variant',
    'atrous_rates', 'encoder_output_stride', 'decoder_output_stride', 'upsample_logits',
    'frag_cls_agnostic', 'frag_loc_agnostic', 'multi_grid', 'logits_kernel_size',
    'image_pyramid', 'add_image_level_feature', 'image_pooling_stride', 'aspp_with_batch_norm',
    'aspp_with_separable_conv', 'depth_multiplier', 'divisible_by',
    'decoder_use_separable_conv', 'merge_method', 'prediction_with_upsampled_logits',
    'use_bounded_activation', 'multi_scale_inference', 'precision', 'frames', 'synthetic',
    'num_objs', 'seed', 'decode_threads', 'prefetch')


def build_parser():
  ap = argparse.ArgumentParser(description=__doc__,
                               formatter_class=argparse.RawTextHelpFormatter)
  for act in infer.build_parser()._actions:
    if act.dest in _SHARED_FLAGS:
      kw = dict(default=act.default, type=act.type, help=act.help, required=act.required)
      if act.choices is not None:
        kw['choices'] = act.choices
      ap.add_argument(*act.option_strings, **kw)
  a = ap.add_argument
  # scripts/eval.py:34-48
  a('--eval_max_height_before_crop', type=int, default=480)
  a('--eval_crop_size', default='640,480')
  a('--eval_interval_secs', type=int, default=3600)
  a('--eval_tfrecord_names', default=None)
  # this build
  a('--eval_frag_labels', default=None,
    help='not in the reference: count fragment hits too (default: true when the model folder '
         'or the store holds fragments)')
  a('--batch_size', type=int, default=1,
    help='not in the reference (fixed at 1 there): images per step')
  return ap


def prepare(argv=None):
  """Parses the command line, applies params.yml and refuses what this build cannot run."""
  args = build_parser().parse_args(argv)
  model_dir = os.path.join(os.environ.get('TF_MODELS_PATH', '.'), args.model)
  infer.update_flags(args, os.path.join(model_dir, infer.PARAMS_FILENAME))   # eval.py:59
  infer.check_supported_flags(args)
  if not (args.dataset and os.environ.get('BOP_PATH')):
    raise ValueError('eval.py needs --dataset and $BOP_PATH (object models)')
  if args.batch_size < 1:
    raise ValueError('--batch_size must be >= 1')
  return args, model_dir


def _frames_args(args):
  """The namespace infer.load_frames reads, with the eval_* flags under its names."""
  ns = argparse.Namespace(**vars(args))
  ns.infer_crop_size = args.eval_crop_size
  ns.infer_tfrecord_names = args.eval_tfrecord_names
  ns.infer_max_height_before_crop = args.eval_max_height_before_crop
  return ns


def read_global_step(checkpoint_path):
  """The checkpoint's global_step variable; 0 for random weights or an .npz checkpoint."""
  if checkpoint_path is None or checkpoint_path.endswith('.npz'):
    return 0
  from epos_amd import tf_checkpoint
  return int(np.asarray(tf_checkpoint.load_checkpoint(
      checkpoint_path, names=['global_step'])['global_step']).reshape(-1)[0])


def main(argv=None):
  args, model_dir = prepare(argv)
  import torch
  from epos_amd import model, multiscale, ply, render, synthetic
  from epos_amd import frames as eframes
  checkpoint_dir = os.path.join(model_dir, 'train')            # eval.py:65
  eval_dir = os.path.join(model_dir, 'eval')                   # eval.py:71-72
  os.makedirs(eval_dir, exist_ok=True)
  dev_index = int(os.environ.get('EPOS_FORCE_DEVICE', 0))
  dev = 'cuda:%d' % dev_index
  torch.cuda.set_device(dev_index)
  ckpt, num_objs, checkpoint_path = infer.load_checkpoint(args, checkpoint_dir)

  last_path = os.path.join(eval_dir, eval_utils.LAST_EVALUATION)
  last = open(last_path).read() if os.path.exists(last_path) else None
  reason = eval_utils.skip_reason(last, checkpoint_path, time.time(), args.eval_interval_secs)
  if reason is not None:
    print(reason)
    return None
  print('Evaluating on: {}'.format(args.eval_tfrecord_names))  # eval.py:94

  store = infer.load_fragments(model_dir, args.num_frags)
  if store is None and not args.synthetic:
    store = infer.fragment_from_bop_models(model_dir, args, dev)
  if store is None:
    if not args.synthetic:
      raise ValueError('fragments.pkl / fragments.npz not found in ' + model_dir +
                       ' and no BOP models under $BOP_PATH/<dataset>/models*')
    store = synthetic.ModelStore(num_objs, args.num_frags, seed=0)
  obj_ids = [o for o in store.dp_model['obj_ids'] if 1 <= o <= num_objs]
  frames, h, w = infer.load_frames(_frames_args(args), num_objs, 0, 1, obj_ids)
  frag_labels = (bool(store.frag_centers) if args.eval_frag_labels is None
                 else infer.str2bool(args.eval_frag_labels))

  # the renderer holds the 'eval' models, as --vis_renderer mesh of infer.py does
  models = ply.load_models(os.environ['BOP_PATH'], args.dataset, 'eval', obj_ids=obj_ids)
  renderer = render.Renderer(dev)
  for o in sorted(models):
    renderer.add_model(o, models[o])
  if frag_labels:
    frag_pool = render.pool_fragments(store.frag_centers, store.frag_sizes, num_objs)
  else:
    frag_pool = (np.zeros((num_objs, 1, 3)), np.ones((num_objs, 1)))

  B = args.batch_size
  pyramid = multiscale.normalize_pyramid(infer._as_list(args.image_pyramid, float) or None)
  mo = model.ModelOptions(
      model.get_outputs_to_num_channels(num_objs, args.num_frags), crop_size=(w, h),
      atrous_rates=infer._as_list(args.atrous_rates, int),
      encoder_output_stride=args.encoder_output_stride,
      decoder_output_stride=infer._as_list(args.decoder_output_stride, int),
      model_variant=args.model_variant, multi_grid=infer._as_list(args.multi_grid, int),
      merge_method=args.merge_method if pyramid is not None else 'max')
  net = model.get_net(ckpt, B, h, w, num_objs, args.num_frags, mo, dev,
                      precision=args.precision, image_pyramid=pyramid)
  out_size = (net.out_w, net.out_h)
  ev = eval_utils.SegmentationEval(num_objs, ignore_label=255, device=dev,
                                   num_frags=args.num_frags if frag_labels else None)
  held_max = 2                                   # batches whose uploads may still be pending
  feed = eframes.Prefetcher(frames, B, h, w, workers=args.decode_threads or None,
                            ahead=max(1, args.prefetch), inflight=held_max)
  if frames:                                     # set-up, not evaluation: kernels and the graph
    net.forward(torch.zeros((B, h, w, 3), dtype=torch.uint8).pin_memory(), use_graph=True)
    torch.cuda.synchronize()

  time_start = time.time()
  held = collections.deque()                     # (event behind the batch's work, i0)
  for i0, chunk, imgs in feed:
    # a staging buffer goes back to the decoders once the step that reads it has run
    while held and (len(held) >= held_max or held[0][0].query()):
      done, j0 = held.popleft()
      done.synchronize()
      feed.release(j0)
    pred = net.forward(imgs, use_graph=True)
    n_real = len(frames[i0:i0 + B])
    maps = [eval_utils.gt_maps_device(renderer, f, out_size, frag_pool, args.dataset,
                                      input_size=(w, h)) for f in chunk[:n_real]]
    gt_obj = torch.stack([m[0] for m in maps])
    if frag_labels:
      ev.update(gt_obj, pred['pred_obj_label'][:n_real], torch.stack([m[1] for m in maps]),
                pred['pred_frag_conf'][:n_real])
    else:
      ev.update(gt_obj, pred['pred_obj_label'][:n_real])
    done = torch.cuda.Event()
    done.record()
    held.append((done, i0))
    if (i0 // B + 1) % 100 == 0:
      print('Evaluating batch {}'.format(i0 // B + 1))         # eval.py:197-205
  torch.cuda.synchronize()
  for _, j0 in held:
    feed.release(j0)
  loop_s = time.time() - time_start

  metrics = ev.write(eval_dir, read_global_step(checkpoint_path))
  with open(last_path, 'w') as f:                              # eval.py:235-241
    json.dump({'time': time.time(), 'checkpoint_path': checkpoint_path}, f)
  print('eval: {} images, miou_all={:.6f}, miou_fg={:.6f}, frag_acc={}, {:.1f} images/s'.format(
      len(frames), metrics['miou_all'], metrics['miou_fg'],
      '{:.6f}'.format(metrics['frag_acc']) if frag_labels else 'n/a',
      len(frames) / max(loop_s, 1e-9)))
  return metrics


if __name__ == '__main__':
  main()
