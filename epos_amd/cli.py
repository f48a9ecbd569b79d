"""What the command-line scripts (infer.py, eval.py, eval_poses.py) share: flag definitions,
params.yml handling, the model folder's checkpoint and fragments, input frames, the network's
ModelOptions, the renderer of the 'eval' models and the staging-buffer bookkeeping of a loop
that keeps several steps in flight. torch is imported where it is needed, so that parsing and
the metadata-only routes run without it."""
import collections
import glob
import json
import os
import pickle

import numpy as np

from epos_amd import synthetic, weights

PARAMS_FILENAME = 'params.yml'   # common.py


def str2bool(v):
  return str(v).lower() in ('1', 'true', 'yes', 'y')


def as_list(v, cast):
  if v is None:
    return None
  if isinstance(v, (list, tuple)):
    return [cast(x) for x in v]
  return [cast(x) for x in str(v).strip('[]()').split(',') if str(x).strip()]


def crop_size(value):
  """(w, h) of a crop-size flag: 'w,h' as on the command line, or the list a params.yml holds."""
  w, h = as_list(value, int)[:2]
  return w, h


def result_suffix(infer_name):
  """'_<infer_name>' in the names of result files; '' without --infer_name."""
  return '' if infer_name is None else '_' + infer_name


def model_dir(args):
  return os.path.join(os.environ.get('TF_MODELS_PATH', '.'), args.model)   # config.py:9-16


def device_from_env(local_rank=0):
  """The device index of this process. EPOS_FORCE_DEVICE=0 maps every rank onto one GPU
  (multi-rank flow on a one-GPU test box, together with EPOS_DIST_BACKEND=gloo), as in
  bench.py."""
  return int(os.environ.get('EPOS_FORCE_DEVICE', local_rank))


def update_flags(args, params_path):
  """common.py:157-177: YAML values override flag DEFAULTS."""
  if not os.path.exists(params_path):
    return
  if os.path.basename(params_path).split('.')[1] not in ['yml', 'yaml']:
    raise ValueError('Only YAML format is currently supported.')
  import yaml
  with open(params_path, 'r') as f:
    params = yaml.safe_load(f) or {}
  for name, val in params.items():
    if hasattr(args, name):
      setattr(args, name, val)


# Flags of common.py:60-154 the network plan implements at ONE value only. A model
# trained with another value has a different graph (other layers, other head layout),
# so running it through this plan would silently produce garbage: raise instead.
_FIXED_FLAGS = [
    ('upsample_logits', False, 'model.py:661-672: logits stay at the decoder stride'),
    ('frag_cls_agnostic', False, 'common.py:198-202: per-object fragment heads only'),
    ('frag_loc_agnostic', False, 'common.py:61-66: per-object fragment heads only'),
    ('logits_kernel_size', 1, 'model.py:428-431'),
    ('add_image_level_feature', True, 'model.py:217-226'),
    ('aspp_with_batch_norm', True, 'model.py:187-199'),
    ('aspp_with_separable_conv', True, 'model.py:243-256'),
    ('decoder_use_separable_conv', True, 'model.py:369-392'),
    ('use_bounded_activation', False, 'model.py:202,317: ReLU, not ReLU6'),
    ('depth_multiplier', 1.0, 'MobileNet only'),
    ('divisible_by', None, 'MobileNet only'),
]


def check_supported_flags(args):
  """Raises NotImplementedError for a known common.py flag set (on the command line
  or by params.yml) to a value this build's network plan does not implement."""
  bad = []
  for name, want, why in _FIXED_FLAGS:
    got = getattr(args, name)
    if isinstance(want, bool):
      got = str2bool(got) if not isinstance(got, bool) else got
    if got != want and not (want is None and got in (None, 'None', '')):
      bad.append('%s=%r (supported: %r; %s)' % (name, getattr(args, name), want, why))
  pyr = as_list(args.image_pyramid, float)
  if pyr not in (None, [], [1.0]):
    if not str2bool(str(getattr(args, 'multi_scale_inference', False))):
      bad.append('image_pyramid=%r (single scale unless --multi_scale_inference=true, '
                 'model.py:545-546,597)' % (args.image_pyramid,))
    else:
      from epos_amd import multiscale
      multiscale.normalize_pyramid(pyr)                       # ValueError if invalid
      multiscale.check_merge_method(args.merge_method)
  if as_list(args.image_pooling_stride, int) not in ([1, 1],):
    bad.append('image_pooling_stride=%r (supported: 1,1)' % (args.image_pooling_stride,))
  if args.model_variant not in weights.VARIANTS:
    bad.append('model_variant=%r (%s)' % (args.model_variant,
                                         ', '.join(sorted(weights.VARIANTS))))
  if int(args.encoder_output_stride) != 8:
    bad.append('encoder_output_stride=%r (supported: 8)' % args.encoder_output_stride)
  if as_list(args.decoder_output_stride, int) != [4]:
    bad.append('decoder_output_stride=%r (supported: 4)' % (args.decoder_output_stride,))
  if bad:
    raise NotImplementedError(
        'flags outside what this build implements (common.py:60-154): ' + '; '.join(bad))


def check_gt_knn_frags(args):
  """args.gt_knn_frags (the command line's, or params.yml's) as an int; ValueError unless
  1 <= gt_knn_frags <= min(num_frags, 4), before a device is touched."""
  from epos_amd import loss
  k = args.gt_knn_frags
  if isinstance(k, bool) or not isinstance(k, int):
    raise ValueError('gt_knn_frags must be an integer, got %r' % (k,))
  return loss.check_knn(k, int(args.num_frags))


# The flags infer.py and eval.py share, in the groups in which both parsers list them (each
# script puts its own flags between the groups: the order of --help is part of the contract).
def add_model_name_flags(ap):
  ap.add_argument('--master', default='', help='accepted and ignored (scripts/infer.py:38-40: '
                  'BNS name of a TensorFlow master)')
  ap.add_argument('--model', required=True)


def add_precision_flags(ap):
  # not in the reference: run the --image_pyramid ("multi-scale mode"). Off by
  # default: the same params.yml key configures multi-scale TRAINING, and S networks per frame
  # are a cost to ask for.
  ap.add_argument('--multi_scale_inference', type=str2bool, default=False)
  # not in the reference: the network's numeric mode ("bf16 mode")
  ap.add_argument('--precision', type=str, default='fp32', choices=['fp32', 'bf16'])


def add_dataset_flags(ap):
  # epos_lib/common.py:60-154 (the model flags the hot path reads)
  ap.add_argument('--dataset', default=None)
  ap.add_argument('--num_frags', type=int, default=64)


def add_network_flags(ap):
  a = ap.add_argument
  a('--model_variant', default='xception_65',
    help='backbone (feature.py:118-129): xception_41, xception_65, xception_71, '
         'resnet_v1_50, resnet_v1_50_beta, resnet_v1_101, resnet_v1_101_beta')
  a('--atrous_rates', default='12,24,36')
  a('--encoder_output_stride', type=int, default=8)
  a('--decoder_output_stride', default='4')
  a('--upsample_logits', type=str2bool, default=False)
  a('--frag_cls_agnostic', type=str2bool, default=False)
  a('--frag_loc_agnostic', type=str2bool, default=False)
  a('--multi_grid', default=None,
    help='e.g. 1,2,4 for the resnet_v1_*_beta checkpoints (common.py:111-115)')
  # common.py:96-154: known to the reference, supported here at their defaults only
  # (check_supported_flags raises otherwise -- a params.yml must not be half-applied)
  a('--logits_kernel_size', type=int, default=1)
  a('--image_pyramid', default=None)
  a('--add_image_level_feature', type=str2bool, default=True)
  a('--image_pooling_stride', default='1,1')
  a('--aspp_with_batch_norm', type=str2bool, default=True)
  a('--aspp_with_separable_conv', type=str2bool, default=True)
  a('--depth_multiplier', type=float, default=1.0)
  a('--divisible_by', type=int, default=None)
  a('--decoder_use_separable_conv', type=str2bool, default=True)
  a('--merge_method', default='max')
  a('--prediction_with_upsampled_logits', type=str2bool, default=True)
  a('--use_bounded_activation', type=str2bool, default=False)


def add_input_flags(ap):
  # this build
  a = ap.add_argument
  a('--frames', default=None, help='directory with frames.json + images')
  a('--synthetic', type=int, default=0, help='number of synthetic frames')
  a('--num_objs', type=int, default=None, help='object channels (default: from the checkpoint)')


def add_decode_flags(ap):
  a = ap.add_argument
  a('--decode_threads', type=int, default=0,
    help='decoder processes working ahead of the GPU (0 = min(8, cores - 2); '
         'EPOS_DECODE_PROCS=0 makes them in-process threads)')
  a('--prefetch', type=int, default=6, help='batches decoded ahead of the GPU')


def find_checkpoint(checkpoint_dir, name):
  if name is not None:
    path = os.path.join(checkpoint_dir, name)
    if not path.endswith('.npz'):
      path += '.npz'
    return path
  cands = sorted(glob.glob(os.path.join(checkpoint_dir, '*.npz')),
                 key=os.path.getmtime)
  return cands[-1] if cands else None


def load_checkpoint(args, checkpoint_dir):
  """(checkpoint dict, num_objs, path): the TensorFlow checkpoint of <model>/train (the latest
  or --checkpoint_name, infer.py:670-674), else an .npz, else -- with --synthetic -- random
  weights (path None)."""
  ckpt_path = find_checkpoint(checkpoint_dir, args.checkpoint_name)
  tf_prefix = None
  if args.checkpoint_name is not None and os.path.exists(
      os.path.join(checkpoint_dir, args.checkpoint_name + '.index')):
    tf_prefix = os.path.join(checkpoint_dir, args.checkpoint_name)
  elif not (ckpt_path and os.path.exists(ckpt_path)):
    from epos_amd import tf_checkpoint
    tf_prefix = tf_checkpoint.latest_checkpoint(checkpoint_dir)  # infer.py:670-674
  if tf_prefix is not None:
    # A TensorFlow checkpoint (model.ckpt-N.index/.data-*), read without TF.
    from epos_amd import tf_checkpoint
    ckpt = tf_checkpoint.to_epos_checkpoint(
        tf_checkpoint.load_checkpoint(tf_prefix))
    return ckpt, ckpt['logits/pred_obj_conf/biases'].shape[0] - 1, tf_prefix
  if ckpt_path and os.path.exists(ckpt_path):
    ckpt = weights.load_npz(ckpt_path)
    return ckpt, ckpt['logits/pred_obj_conf/biases'].shape[0] - 1, ckpt_path
  if args.synthetic:
    num_objs = args.num_objs or 21
    ckpt = weights.random_init(args.model_variant, num_objs=num_objs,
                               num_frags=args.num_frags, seed=0, randomize_bn=True)
    return ckpt, num_objs, None
  raise ValueError('No checkpoint (.npz) found in {}'.format(checkpoint_dir))


def load_fragments(model_dir, num_frags):
  """fragments.pkl (datagen.py:254-268) or fragments.npz."""
  pkl = os.path.join(model_dir, 'fragments.pkl')
  npz = os.path.join(model_dir, 'fragments.npz')
  if os.path.exists(pkl):
    with open(pkl, 'rb') as f:
      fr = pickle.load(f)
    centers, sizes = fr['frag_centers'], fr['frag_sizes']
  elif os.path.exists(npz):
    z = np.load(npz)
    centers = {int(o): z['frag_centers'][i] for i, o in enumerate(z['obj_ids'])}
    sizes = {int(o): z['frag_sizes'][i] for i, o in enumerate(z['obj_ids'])}
  else:
    return None
  for o in centers:                                   # datagen.py:264-268
    if centers[o].shape[0] != num_frags or sizes[o].shape[0] != num_frags:
      raise ValueError('The loaded fragmentation is not valid.')
  store = synthetic.ModelStore(0, num_frags)
  store.dp_model = {'obj_ids': sorted(int(o) for o in centers)}
  store.frag_centers = {int(o): np.asarray(v, np.float64) for o, v in centers.items()}
  store.frag_sizes = {int(o): np.asarray(v, np.float64) for o, v in sizes.items()}
  return store


def fragment_from_bop_models(model_dir, args, dev):
  """datagen.py:238-296: no fragments.pkl yet -> load the object models of the
  dataset (<BOP_PATH>/<dataset>/models[_<type>]/obj_XXXXXX.ply; 'reconst' for T-LESS,
  'dense' for ITODD, 'eval' for TUD-L, the original ones otherwise), fragment them by
  furthest-point sampling on the GPU, save fragments.pkl next to params.yml."""
  from epos_amd import fragment, ply
  dataset = args.dataset
  bop = os.environ.get('BOP_PATH')
  if not dataset or not bop or dataset not in ply.BOP_OBJ_IDS:
    return None
  mtype = {'tless': 'reconst', 'itodd': 'dense', 'tudl': 'eval'}.get(dataset)
  if not os.path.exists(ply.model_path(bop, dataset, ply.BOP_OBJ_IDS[dataset][0], mtype)):
    return None
  models = ply.load_models(bop, dataset, mtype)
  centers, sizes = fragment.fragment_models(
      {o: m['pts'] for o, m in models.items()}, args.num_frags, device=dev)
  fragment.save_fragments(os.path.join(model_dir, 'fragments.pkl'), centers, sizes)
  return load_fragments(model_dir, args.num_frags)


def resolve_store(model_dir, args, num_objs, dev):
  """The model store: the folder's fragments, else the dataset's models fragmented on the
  device, else -- with --synthetic -- a seeded synthetic store."""
  store = load_fragments(model_dir, args.num_frags)
  if store is None and not args.synthetic:
    store = fragment_from_bop_models(model_dir, args, dev)
  if store is None:
    if not args.synthetic:
      raise ValueError('fragments.pkl / fragments.npz not found in ' + model_dir +
                       ' and no BOP models under $BOP_PATH/<dataset>/models*')
    store = synthetic.ModelStore(num_objs, args.num_frags, seed=0)
  return store


def read_frames_json(frames_dir):
  with open(os.path.join(frames_dir, 'frames.json')) as f:
    return json.load(f)


def load_frames(tfrecord_names, frames_dir, synthetic_count, crop, max_height_before_crop, seed,
                num_objs, rank=0, world=1, obj_ids=None, pixels=True, meta=None):
  """Returns this rank's list of epos_amd.frames.Frame (ids, K, targets known; pixels decoded
  on demand by the prefetcher's threads), plus the frame height and width. crop: a crop-size
  flag (crop_size). pixels=False: metadata only -- frames of a --frames directory open no image
  file and their entries need no ``path``. meta: the entries of <frames_dir>/frames.json where
  the caller has read them already (read_frames_json)."""
  from epos_amd import dist as edist, frames as eframes
  w, h = crop_size(crop)
  if tfrecord_names:
    # <TF_DATA_PATH>/<name>.tfrecord for each name (infer.py:581-583,
    # datagen.py:707-723), read without TensorFlow (epos_amd/tfrecord.py).
    names = tfrecord_names
    if not isinstance(names, (list, tuple)):
      names = [n for n in str(names).split(',') if n]
    data_path = os.environ.get('TF_DATA_PATH', '.')
    paths = []
    for name in names:
      path = os.path.join(data_path, name + '.tfrecord')
      if not os.path.exists(path):
        raise ValueError('No input files: {}'.format(path))   # datagen.py:720-721
      paths.append(path)
    # min_visib_fract=None: the reference builds its inference Dataset without a
    # visibility filter (scripts/infer.py:614), every annotated instance is a target
    frames = eframes.scan_tfrecords(
        paths, (w, h), max_height_before_crop, obj_ids if obj_ids else None, crop_seed=seed)
    b, e = edist.shard_range(len(frames), rank, world)
    frames = frames[b:e]
  elif frames_dir:
    if meta is None:
      meta = read_frames_json(frames_dir)
    b, e = edist.shard_range(len(meta), rank, world)
    frames = eframes.frames_from_dir(frames_dir, meta[b:e], h, w, pixels=pixels)
  elif synthetic_count:
    b, e = edist.shard_range(synthetic_count, rank, world)
    frames = eframes.synthetic_frames(range(b, e), h, w, num_objs, 5)
  else:
    raise ValueError(
        'No input files: give --infer_tfrecord_names, --frames <dir> or '
        '--synthetic N.')
  return frames, h, w


def model_options(args, num_objs, w, h, pyramid):
  from epos_amd import model
  return model.ModelOptions(
      model.get_outputs_to_num_channels(num_objs, args.num_frags), crop_size=(w, h),
      atrous_rates=as_list(args.atrous_rates, int),
      encoder_output_stride=args.encoder_output_stride,
      decoder_output_stride=as_list(args.decoder_output_stride, int),
      model_variant=args.model_variant, multi_grid=as_list(args.multi_grid, int),
      merge_method=args.merge_method if pyramid is not None else 'max')


def eval_renderer(models, dev):
  """A render.Renderer holding `models` ({obj_id: {'pts', 'faces'}}, the 'eval' models of the
  dataset), added in the order of their ids."""
  from epos_amd import render
  renderer = render.Renderer(dev)
  for o in sorted(models):
    renderer.add_model(o, models[o])
  return renderer


def steps_released_in_order(feed, limit):
  """Yields the prefetcher's steps (i0, chunk, imgs) for a loop that enqueues each step's work
  on the current stream. At most `limit` steps' staging buffers stay pending; each goes back
  to the decoders (feed.release), oldest first, once the event behind its step has fired."""
  import torch
  held = collections.deque()                     # (event behind the step's work, i0)
  for i0, chunk, imgs in feed:
    while held and (len(held) >= limit or held[0][0].query()):
      done, j0 = held.popleft()
      done.synchronize()
      feed.release(j0)
    yield i0, chunk, imgs
    done = torch.cuda.Event()
    done.record()
    held.append((done, i0))
  torch.cuda.synchronize()
  for _, j0 in held:
    feed.release(j0)
