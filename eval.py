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
import json
import os
import sys
import time

import numpy as np     # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from epos_amd import cli, eval_utils   # noqa: E402


def build_parser():
  ap = argparse.ArgumentParser(description=__doc__,
                               formatter_class=argparse.RawTextHelpFormatter)
  a = ap.add_argument
  # the model flags of epos_lib/common.py and this build's input / precision options, as
  # infer.py defines them
  cli.add_model_name_flags(ap)
  a('--checkpoint_name', default=None)
  cli.add_precision_flags(ap)
  cli.add_dataset_flags(ap)
  cli.add_network_flags(ap)
  cli.add_input_flags(ap)
  a('--seed', type=int, default=0)
  cli.add_decode_flags(ap)
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
  model_dir = cli.model_dir(args)
  cli.update_flags(args, os.path.join(model_dir, cli.PARAMS_FILENAME))   # eval.py:59
  cli.check_supported_flags(args)
  if not (args.dataset and os.environ.get('BOP_PATH')):
    raise ValueError('eval.py needs --dataset and $BOP_PATH (object models)')
  if args.batch_size < 1:
    raise ValueError('--batch_size must be >= 1')
  return args, model_dir


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
  from epos_amd import model, multiscale, ply, render
  from epos_amd import frames as eframes
  checkpoint_dir = os.path.join(model_dir, 'train')            # eval.py:65
  eval_dir = os.path.join(model_dir, 'eval')                   # eval.py:71-72
  os.makedirs(eval_dir, exist_ok=True)
  dev_index = cli.device_from_env()
  dev = 'cuda:%d' % dev_index
  torch.cuda.set_device(dev_index)
  ckpt, num_objs, checkpoint_path = cli.load_checkpoint(args, checkpoint_dir)

  last_path = os.path.join(eval_dir, eval_utils.LAST_EVALUATION)
  last = open(last_path).read() if os.path.exists(last_path) else None
  reason = eval_utils.skip_reason(last, checkpoint_path, time.time(), args.eval_interval_secs)
  if reason is not None:
    print(reason)
    return None
  print('Evaluating on: {}'.format(args.eval_tfrecord_names))  # eval.py:94

  store = cli.resolve_store(model_dir, args, num_objs, dev)
  obj_ids = [o for o in store.dp_model['obj_ids'] if 1 <= o <= num_objs]
  frames, h, w = cli.load_frames(
      args.eval_tfrecord_names, args.frames, args.synthetic, args.eval_crop_size,
      args.eval_max_height_before_crop, args.seed, num_objs, obj_ids=obj_ids)
  frag_labels = (bool(store.frag_centers) if args.eval_frag_labels is None
                 else cli.str2bool(args.eval_frag_labels))

  # the renderer holds the 'eval' models, as --vis_renderer mesh of infer.py does
  renderer = cli.eval_renderer(
      ply.load_models(os.environ['BOP_PATH'], args.dataset, 'eval', obj_ids=obj_ids), dev)
  if frag_labels:
    frag_pool = render.pool_fragments(store.frag_centers, store.frag_sizes, num_objs)
  else:
    frag_pool = (np.zeros((num_objs, 1, 3)), np.ones((num_objs, 1)))

  B = args.batch_size
  pyramid = multiscale.normalize_pyramid(cli.as_list(args.image_pyramid, float) or None)
  net = model.get_net(ckpt, B, h, w, num_objs, args.num_frags,
                      cli.model_options(args, num_objs, w, h, pyramid), dev,
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
  # a staging buffer goes back to the decoders once the step that reads it has run
  for i0, chunk, imgs in cli.steps_released_in_order(feed, held_max):
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
    if (i0 // B + 1) % 100 == 0:
      print('Evaluating batch {}'.format(i0 // B + 1))         # eval.py:197-205
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
