#!/usr/bin/env python
"""Fine-tunes the three logits layers of an EPOS checkpoint on MI355X and, when
--freeze_regex_list leaves it free, decoder/decoder_conv1_pointwise below them.

    python train_heads.py --model=<model_name> --train_tfrecord_names=<n> --dataset <d> [flags]

The part of the reference's ``scripts/train.py`` that this build has kernels for: the losses
(epos_lib/loss.py:99-303), the gradients of logits/pred_obj_conf, pred_frag_conf and
pred_frag_loc, tf.train.MomentumOptimizer with the l2 regulariser and the last-layer gradient
multiplier (train.py:340-384) and the learning-rate schedules (train_utils.py:117-195).
By default everything below the logits stays frozen, as the reference does with
--freeze_regex_list. A list that leaves variables of decoder/decoder_conv1_pointwise trainable
(its weights, BatchNorm/gamma, BatchNorm/beta: --freeze_regex_list
'^(?!logits|decoder/decoder_conv1_pointwise)') trains them too, with the batch-norm statistics
frozen (epos_amd/trainer.py); any other unfrozen scope is refused. No
batch-norm statistics, one device, fp32, one scale. --gt_knn_frags (train.py:82; default 1, at
most 4 and no more than --num_frags) assigns every pixel to its k nearest fragments, and the two
fragment losses run over the (pixel, fragment) rows. --data_augmentations (a mapping in the YAML
format, on the command line or in params.yml, datagen.py:629-670) runs on the device between
the upload of a batch and its forward pass (epos_amd/augment.py); its draws are keyed by
(--seed, global step, image), so a resumed run augments as an uninterrupted one would.

  * env TF_DATA_PATH / TF_MODELS_PATH / BOP_PATH; <TF_MODELS_PATH>/<model>/params.yml overrides
    flag defaults; the flags of scripts/train.py:53-149 under their names and defaults;
  * annotated frames from ``--train_tfrecord_names a,b``; ``--frames <dir>`` (frames.json with
    gt_poses) and ``--synthetic N`` work as in ``eval_loss.py``. The frames are visited in their
    order, again and again, until --train_steps: step s trains on the frames
    (s * train_batch_size + b) mod N -- no shuffling, so a resumed run continues the cycle;
  * weights from <model>/train/ as ``infer.py`` finds them. A TensorFlow checkpoint is read
    whole: its '/Momentum' slots and global_step too, so a run started again on a folder this
    script wrote into resumes where the last checkpoint stopped;
  * output: <model>/train/model.ckpt-<global_step> (.index, .data-00000-of-00001) with every
    variable of the loaded checkpoint, the six logits variables (and the trained variables of
    decoder/decoder_conv1_pointwise) replaced, their '/Momentum' slots and an int64
    global_step, every --save_interval_steps and at the end;
    the ``checkpoint`` state file names the newest; one TensorBoard event file per run with
    train/obj_cls_loss, train/frag_cls_loss, train/frag_loc_loss and train/total_loss every
    --log_steps, and one line per log step on stdout.

Each step is enqueued without waiting for the device (trainer.train_step). At every log
step and before every save the run reads back what the steps since the last look left behind:
the weight packer's status words and the counts of pixels with non-finite logits. If the
packer refused an update (non-finite weights: the run has diverged) the run ends with exit
status 1 and writes no checkpoint of those weights.
"""
import argparse
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from epos_amd import cli, eval_utils, trainer   # noqa: E402
from epos_amd import weights as W   # noqa: E402


def build_parser():
  ap = argparse.ArgumentParser(description=__doc__,
                               formatter_class=argparse.RawTextHelpFormatter)
  a = ap.add_argument
  # the flag groups of eval_loss.py
  cli.add_model_name_flags(ap)
  a('--checkpoint_name', default=None)
  cli.add_precision_flags(ap)
  cli.add_dataset_flags(ap)
  cli.add_network_flags(ap)
  cli.add_input_flags(ap)
  a('--seed', type=int, default=0)
  cli.add_decode_flags(ap)
  # scripts/train.py:53-149
  a('--log_steps', type=int, default=100)
  a('--save_interval_steps', type=int, default=50000)
  a('--obj_cls_loss_weight', type=float, default=1.0)
  a('--frag_cls_loss_weight', type=float, default=1.0)
  a('--frag_loc_loss_weight', type=float, default=100.0)
  a('--gt_knn_frags', type=int, default=1,
    help='fragments a pixel is assigned to (train.py:82), 1..min(num_frags, 4)')
  a('--freeze_regex_list', action='append', default=None,
    help='accepted when every variable it leaves trainable below the logits belongs to '
         'decoder/decoder_conv1_pointwise; default: everything below the logits frozen')
  a('--learning_policy', default='poly', choices=['poly', 'step'])
  a('--base_learning_rate', type=float, default=0.0001)
  a('--learning_rate_decay_factor', type=float, default=0.1)
  a('--learning_rate_decay_step', type=int, default=2000)
  a('--learning_power', type=float, default=0.9)
  a('--train_steps', type=int, default=2000000)
  a('--momentum', type=float, default=0.9)
  a('--train_batch_size', type=int, default=1)
  a('--weight_decay', type=float, default=0.00004)
  a('--train_max_height_before_crop', type=int, default=480)
  a('--train_crop_size', default='640,480')
  a('--last_layer_gradient_multiplier', type=float, default=1.0)
  a('--last_layers_contain_logits_only', type=cli.str2bool, default=False)
  a('--slow_start_step', type=int, default=0)
  a('--slow_start_learning_rate', type=float, default=0.0001)
  a('--fine_tune_batch_norm', type=cli.str2bool, default=False)
  a('--train_tfrecord_names', default=None)
  a('--data_augmentations', default=None)
  return ap


TRAINABLE_OF_KIND = {'conv': ('weights', 'BatchNorm/gamma', 'BatchNorm/beta'),
                     'dw': ('depthwise_weights', 'BatchNorm/gamma', 'BatchNorm/beta')}


def unfrozen_below_logits(regexes, args):
  """The trainable variables below the logits that none of `regexes` freezes, in the network's
  order: the reference filters per variable name (train.py:369-371)."""
  names = []
  for kind, scope, _, _ in W.variable_specs(
      args.model_variant, 1, args.num_frags, tuple(cli.as_list(args.atrous_rates, int))):
    if scope.startswith('logits/'):
      continue
    for v in TRAINABLE_OF_KIND[kind]:
      name = scope + '/' + v
      if not any(re.search(r, name) for r in regexes):
        names.append(name)
  return names


def prepare(argv=None):
  """Parses the command line, applies params.yml and refuses what this build cannot train.
  args.data_augmentations becomes augment.parse's list."""
  from epos_amd import augment, multiscale
  args = build_parser().parse_args(argv)
  model_dir = cli.model_dir(args)
  cli.update_flags(args, os.path.join(model_dir, cli.PARAMS_FILENAME))
  cli.check_supported_flags(args)
  if args.precision != 'fp32':
    raise NotImplementedError('--precision %s: train_heads.py trains in fp32 only' %
                              args.precision)
  if multiscale.normalize_pyramid(cli.as_list(args.image_pyramid, float) or None) is not None:
    raise NotImplementedError('image_pyramid=%r: train_heads.py trains a single-scale network' %
                              (args.image_pyramid,))
  if cli.str2bool(args.fine_tune_batch_norm):
    raise NotImplementedError('fine_tune_batch_norm=true: the batch-norm layers lie below the '
                              'logits and stay frozen')
  args.data_augmentations = augment.parse(args.data_augmentations)
  args.layer_trainable = ()          # the variables of decoder_conv1_pointwise to train
  if args.freeze_regex_list is not None:
    regexes = args.freeze_regex_list
    regexes = [regexes] if isinstance(regexes, str) else list(regexes)
    free = unfrozen_below_logits(regexes, args)
    other = [n for n in free if n not in trainer.VARIABLES]
    if other:
      raise NotImplementedError(
          'freeze_regex_list=%r leaves %s trainable: train_heads.py trains the logits layers '
          'and %s only' % (regexes, other[0], ', '.join(
              s for s in W.TRAINABLE_LAYERS if s not in W.LOGITS_LAYERS)))
    args.layer_trainable = tuple(free)
  if not (args.dataset and os.environ.get('BOP_PATH')):
    raise ValueError('train_heads.py needs --dataset and $BOP_PATH (object models)')
  if args.train_batch_size < 1:
    raise ValueError('--train_batch_size must be >= 1')
  if args.log_steps < 1 or args.save_interval_steps < 1:
    raise ValueError('--log_steps and --save_interval_steps must be >= 1')
  args.gt_knn_frags = cli.check_gt_knn_frags(args)
  return args, model_dir


def schedule(args, step):
  return trainer.learning_rate(
      step, args.learning_policy, args.base_learning_rate, args.learning_rate_decay_step,
      args.learning_rate_decay_factor, args.train_steps, args.learning_power,
      args.slow_start_step, args.slow_start_learning_rate)


def save(checkpoint_dir, raw, opt, step):
  """model.ckpt-<step> and the ``checkpoint`` state file naming it."""
  import numpy as np
  from epos_amd import tf_checkpoint
  variables = dict(raw)
  variables.update(opt.state())
  variables['global_step'] = np.asarray(step, np.int64)
  os.makedirs(checkpoint_dir, exist_ok=True)
  name = 'model.ckpt-%d' % step
  tf_checkpoint.write_checkpoint(os.path.join(checkpoint_dir, name), variables)
  with open(os.path.join(checkpoint_dir, 'checkpoint'), 'w') as f:
    f.write('model_checkpoint_path: "%s"\nall_model_checkpoint_paths: "%s"\n' % (name, name))
  return name


def main(argv=None):
  args, model_dir = prepare(argv)
  import torch
  from epos_amd import augment, loss, model, ply, render, tf_checkpoint, tf_events
  from epos_amd import frames as eframes
  checkpoint_dir = os.path.join(model_dir, 'train')
  dev_index = cli.device_from_env()
  dev = 'cuda:%d' % dev_index
  torch.cuda.set_device(dev_index)
  ckpt, num_objs, checkpoint_path = cli.load_checkpoint(args, checkpoint_dir)
  raw = dict(ckpt)
  if checkpoint_path and os.path.exists(checkpoint_path + '.index'):
    raw = tf_checkpoint.load_checkpoint(checkpoint_path)     # the slots and global_step too
  step = int(raw.get('global_step', 0))
  print('Training on: {} (from step {})'.format(args.train_tfrecord_names, step))

  store = cli.resolve_store(model_dir, args, num_objs, dev)
  if not store.frag_centers:
    raise ValueError('the fragment losses need the fragmentation of the model folder')
  obj_ids = [o for o in store.dp_model['obj_ids'] if 1 <= o <= num_objs]
  frames, h, w = cli.load_frames(
      args.train_tfrecord_names, args.frames, args.synthetic, args.train_crop_size,
      args.train_max_height_before_crop, args.seed, num_objs, obj_ids=obj_ids)
  if not frames:
    raise ValueError('no frames to train on')
  renderer = cli.eval_renderer(
      ply.load_models(os.environ['BOP_PATH'], args.dataset, 'eval', obj_ids=obj_ids), dev)
  frag_pool = render.pool_fragments(store.frag_centers, store.frag_sizes, num_objs)

  B = args.train_batch_size
  net = model.get_net(ckpt, B, h, w, num_objs, args.num_frags,
                      cli.model_options(args, num_objs, w, h, None), dev)
  out_size = (net.out_w, net.out_h)
  opt = trainer.Optimizer(
      raw, args.base_learning_rate, args.momentum, args.weight_decay,
      args.last_layer_gradient_multiplier, cli.str2bool(args.last_layers_contain_logits_only),
      trainable=loss.HEAD_VARIABLES + args.layer_trainable, device=dev)
  if args.layer_trainable:
    print('Training below the logits: {}'.format(', '.join(args.layer_trainable)))
  augmenter = None
  if args.data_augmentations:
    augmenter = augment.Augmenter(args.data_augmentations, args.seed, dev)
    print('Augmentations: {}'.format(', '.join(augmenter.names)))
  weights = (args.obj_cls_loss_weight, args.frag_cls_loss_weight, args.frag_loc_loss_weight)
  todo = max(0, args.train_steps - step)
  order = [frames[(s * B + b) % len(frames)] for s in range(step, step + todo) for b in range(B)]
  held_max = 2
  feed = eframes.Prefetcher(order, B, h, w, workers=args.decode_threads or None,
                            ahead=max(1, args.prefetch), inflight=held_max)
  # what the steps since the last look left behind, on the device (refused: sized by the first
  # step's status words)
  refused = None
  bad_pixels = torch.zeros((), dtype=torch.int64, device=dev)
  events = tf_events.EventWriter(checkpoint_dir) if todo else None

  def look(values, lr):
    """Synchronises. Ends the run when an update was refused or logits were not finite."""
    n_refused, n_bad = int(refused.ne(0).sum().item()), int(bad_pixels.item())
    if n_refused or n_bad:
      print('train_heads: stopping at step {}: the weight packer refused {} matrices, {} pixels '
            'had non-finite logits; the last checkpoint stays the newest'.format(
                step, n_refused, n_bad))
      sys.exit(1)
    return [float(v) for v in values.cpu()]

  time_start, saved = time.time(), None
  for _, chunk, imgs in cli.steps_released_in_order(feed, held_max):
    fields = [eval_utils.gt_loss_fields_device(renderer, f, out_size, frag_pool, args.dataset,
                                               input_size=(w, h),
                                               knn_frags=args.gt_knn_frags) for f in chunk]
    gt = {k: torch.stack([f[k] for f in fields]) for k in loss.GT_KEYS}
    lr = schedule(args, step)
    values, bad, status = trainer.train_step(net, imgs, gt, opt, lr, weights,
                                             augment=augmenter, step=step)
    refused = status.clone() if refused is None else refused.bitwise_or_(status)
    bad_pixels.add_(bad.sum())
    step += 1
    last = step == args.train_steps
    if step % args.log_steps == 0 or last:
      v = look(values, lr)
      events.add(list(zip(('train/' + n for n in loss.NAMES), v)), step)
      print('step {}: lr={:.6g}, obj_cls={:.6f}, frag_cls={:.6f}, frag_loc={:.6f}, '
            'total={:.6f}, {:.2f} s'.format(step, lr, v[0], v[1], v[2], v[3],
                                            time.time() - time_start))
    if step % args.save_interval_steps == 0 or last:
      look(values, lr)
      saved = save(checkpoint_dir, raw, opt, step)
  print('train_heads: {} steps, global_step={}, {}'.format(
      todo, step, 'wrote ' + saved if saved else 'nothing to do'))
  return step


if __name__ == '__main__':
  main()
