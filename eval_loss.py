#!/usr/bin/env python
"""The validation value of the three EPOS training losses on MI355X.

    python eval_loss.py --model=<model_name> --eval_tfrecord_names=<n> --dataset <d> [flags]

The reference has no script for this: it computes the losses inside ``scripts/train.py``
(epos_lib/loss.py:99-303, train.py:198-235) -- the object cross-entropy, the fragment
cross-entropy and the fragment-localisation Huber loss, weighted by --obj_cls_loss_weight,
--frag_cls_loss_weight and --frag_loc_loss_weight (train.py:72-80; a training params.yml
supplies them). This script evaluates them for a checkpoint on annotated frames, with the
contract of ``eval.py``:
  * env TF_DATA_PATH / TF_MODELS_PATH / BOP_PATH; <TF_MODELS_PATH>/<model>/params.yml overrides
    flag defaults; weights from <model>/train/ as ``infer.py`` finds them;
  * annotated frames from ``--eval_tfrecord_names a,b``; ``--frames <dir>`` (frames.json with
    gt_poses) and ``--synthetic N`` work as in ``eval.py``;
  * results in <model>/eval_loss/: losses_<global_step>.json (mean, pooled, per_object, the
    weights, the number of images and per_image keyed 'scene_id/im_id') and a TensorBoard event
    file with eval/obj_cls_loss, eval/frag_cls_loss, eval/frag_loc_loss and eval/total_loss
    (the means over the images). There is no skip logic: a rerun overwrites.

total_loss is the sum of the three weighted losses WITHOUT the regularisation term that
train.py:280 adds (epos_amd/loss.py; DESIGN.md, "Losses").

The ground-truth fields are rendered on the device from the object meshes with the
--gt_knn_frags nearest fragments per pixel (train.py:82; default 1, at most 4 and no more than
--num_frags; a training params.yml supplies it; with more than one, losses_<global_step>.json
carries a gt_knn_frags key), so the run needs --dataset
and $BOP_PATH with the 'eval' models. The network runs without its softmax (raw logits); each
batch's forward pass, ground-truth fields and loss sums are enqueued on one stream and one row
of numbers per image is downloaded at the end. A single-scale network only: the reference adds
one loss per scale of a pyramid, which is a training-time meaning.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from epos_amd import cli, eval_utils   # noqa: E402


def build_parser():
  ap = argparse.ArgumentParser(description=__doc__,
                               formatter_class=argparse.RawTextHelpFormatter)
  a = ap.add_argument
  # the flag groups of eval.py
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
  a('--eval_tfrecord_names', default=None)
  # scripts/train.py:72-80
  a('--obj_cls_loss_weight', type=float, default=1.0)
  a('--frag_cls_loss_weight', type=float, default=1.0)
  a('--frag_loc_loss_weight', type=float, default=100.0)
  a('--gt_knn_frags', type=int, default=1,
    help='fragments a pixel is assigned to (train.py:82), 1..min(num_frags, 4)')
  # this build
  a('--batch_size', type=int, default=1, help='images per step')
  return ap


def prepare(argv=None):
  """Parses the command line, applies params.yml and refuses what this build cannot run."""
  from epos_amd import multiscale
  args = build_parser().parse_args(argv)
  model_dir = cli.model_dir(args)
  cli.update_flags(args, os.path.join(model_dir, cli.PARAMS_FILENAME))
  cli.check_supported_flags(args)
  if multiscale.normalize_pyramid(cli.as_list(args.image_pyramid, float) or None) is not None:
    raise NotImplementedError(
        'eval_loss.py runs a single-scale network: the reference adds one loss per scale of '
        'image_pyramid=%r, which is a training-time meaning' % (args.image_pyramid,))
  if not (args.dataset and os.environ.get('BOP_PATH')):
    raise ValueError('eval_loss.py needs --dataset and $BOP_PATH (object models)')
  if args.batch_size < 1:
    raise ValueError('--batch_size must be >= 1')
  args.gt_knn_frags = cli.check_gt_knn_frags(args)
  return args, model_dir


def main(argv=None):
  args, model_dir = prepare(argv)
  import torch
  from epos_amd import loss, model, ply, render
  from epos_amd import frames as eframes
  import eval as eval_script          # read_global_step
  checkpoint_dir = os.path.join(model_dir, 'train')
  out_dir = os.path.join(model_dir, 'eval_loss')
  dev_index = cli.device_from_env()
  dev = 'cuda:%d' % dev_index
  torch.cuda.set_device(dev_index)
  ckpt, num_objs, checkpoint_path = cli.load_checkpoint(args, checkpoint_dir)
  print('Evaluating on: {}'.format(args.eval_tfrecord_names))

  store = cli.resolve_store(model_dir, args, num_objs, dev)
  if not store.frag_centers:
    raise ValueError('the fragment losses need the fragmentation of the model folder')
  obj_ids = [o for o in store.dp_model['obj_ids'] if 1 <= o <= num_objs]
  frames, h, w = cli.load_frames(
      args.eval_tfrecord_names, args.frames, args.synthetic, args.eval_crop_size,
      args.eval_max_height_before_crop, args.seed, num_objs, obj_ids=obj_ids)
  renderer = cli.eval_renderer(
      ply.load_models(os.environ['BOP_PATH'], args.dataset, 'eval', obj_ids=obj_ids), dev)
  frag_pool = render.pool_fragments(store.frag_centers, store.frag_sizes, num_objs)

  B = args.batch_size
  net = model.get_net(ckpt, B, h, w, num_objs, args.num_frags,
                      cli.model_options(args, num_objs, w, h, None), dev,
                      precision=args.precision)
  out_size = (net.out_w, net.out_h)
  ev = loss.LossEval(num_objs, args.num_frags, dev, args.obj_cls_loss_weight,
                     args.frag_cls_loss_weight, args.frag_loc_loss_weight, ignore_label=255,
                     knn=args.gt_knn_frags)
  held_max = 2                                   # batches whose uploads may still be pending
  feed = eframes.Prefetcher(frames, B, h, w, workers=args.decode_threads or None,
                            ahead=max(1, args.prefetch), inflight=held_max)
  if frames:                                     # set-up, not evaluation: kernels and the graph
    net.forward_logits(torch.zeros((B, h, w, 3), dtype=torch.uint8).pin_memory(),
                       use_graph=True)
    torch.cuda.synchronize()

  time_start = time.time()
  for i0, chunk, imgs in cli.steps_released_in_order(feed, held_max):
    logits = net.forward_logits(imgs, use_graph=True)
    n_real = len(frames[i0:i0 + B])
    fields = [eval_utils.gt_loss_fields_device(renderer, f, out_size, frag_pool, args.dataset,
                                               input_size=(w, h),
                                               knn_frags=args.gt_knn_frags)
              for f in chunk[:n_real]]
    ev.update({k: v[:n_real] for k, v in logits.items()},
              {k: torch.stack([f[k] for f in fields]) for k in loss.GT_KEYS})
    if (i0 // B + 1) % 100 == 0:
      print('Evaluating batch {}'.format(i0 // B + 1))
  loop_s = time.time() - time_start

  keys = ['{}/{}'.format(f.scene_id, f.im_id) for f in frames]
  res = ev.write(out_dir, eval_script.read_global_step(checkpoint_path), keys)
  m = res['mean']
  print('eval_loss: {} images, obj_cls={:.6f}, frag_cls={:.6f}, frag_loc={:.6f}, total={:.6f}, '
        '{:.1f} images/s'.format(len(frames), m['obj_cls_loss'], m['frag_cls_loss'],
                                 m['frag_loc_loss'], m['total_loss'],
                                 len(frames) / max(loop_s, 1e-9)))
  return res


if __name__ == '__main__':
  main()
