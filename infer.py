#!/usr/bin/env python
"""EPOS inference on MI355X -- drop-in for ``scripts/infer.py`` of thodan/epos.

    python infer.py --model=<model_name> [flags]                       (infer.py:6-8)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 \
        --master-addr 127.0.0.1 infer.py --model=<model_name> ...

Same contract as the reference script:
  * env TF_DATA_PATH / TF_MODELS_PATH / BOP_PATH (config.py:9-16);
  * <TF_MODELS_PATH>/<model>/params.yml overrides flag defaults (common.py:157-177,
    list-valued crop sizes parsed from "w,h" strings);
  * weights from <model>/train/ -- the TensorFlow checkpoint itself
    (model.ckpt-N.index/.data-*, latest or --checkpoint_name, read without
    TensorFlow by epos_amd/tf_checkpoint.py) or an ``.npz`` keyed by the TF
    variable names; fragments from <model>/fragments.pkl
    (datagen.py:254-268) or <model>/fragments.npz;
  * poses written to <model>/infer/estimated-poses[_<infer_name>].csv in BOP'19
    format (infer.py:753-760); optional corr_*/NNNNNN_corr_OO.txt (infer.py:294-345).

Input frames: ``--infer_tfrecord_names a,b`` reads <TF_DATA_PATH>/<name>.tfrecord
like the reference (infer.py:581-583) but without TensorFlow (epos_amd/tfrecord.py:
TFRecord framing + tf.Example parsing + PIL decoding; frames that would need the
reference's resize raise). Alternatively ``--frames <dir>`` holding ``frames.json``
(list of {scene_id, im_id, path, K[9], targets {obj_id: count}, optionally gt_poses
[{obj_id, R[9], t[3]}] for --vis}) + images (.npy
HxWx3 or anything PIL reads), or ``--synthetic N`` seeded synthetic frames.

Reference quirks kept on purpose: only the *localization* task has targets (the
reference dereferences gt_poses=None in detection mode, infer.py:400); here
--task_type=detection fits every object of the model store with unlimited
instances. ``infer_crop_size`` is (width, height) as consumed by the reference
(datagen.py:448-449), despite its help string.
"""
import argparse
import collections
import os
import sys
import time
import types

import numpy as np     # noqa: E402
import torch           # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from epos_amd import bop_io, cli, dist as edist, eval_utils, fitting, pipeline   # noqa: E402
from epos_amd import multiscale                                                  # noqa: E402


# "all found" (num_instances = -1, detection) needs a bound for the static buffers
# (--detection_instance_cap); every (frame, object) that reaches it is reported
# (EposPipeline.cap_hits, printed per frame and summed up at the end of the run). This is a
# DEVIATION from the reference, where -1 is unbounded (scripts/infer.py:463-468:
# min(-1, max_instances_to_fit) == -1, so that flag never limits detection either -- nor
# does it here).
DETECTION_INSTANCE_CAP = 16


def build_parser():
  ap = argparse.ArgumentParser(description=__doc__,
                               formatter_class=argparse.RawTextHelpFormatter)
  a = ap.add_argument
  str2bool = cli.str2bool
  # scripts/infer.py:37-120
  cli.add_model_name_flags(ap)
  a('--cpu_only', type=str2bool, default=False)
  a('--task_type', default=pipeline.LOCALIZATION)
  a('--infer_tfrecord_names', default=None)
  a('--infer_max_height_before_crop', type=int, default=480)
  a('--infer_crop_size', default='640,480')
  a('--checkpoint_name', default=None)
  a('--project_to_surface', type=str2bool, default=False)
  a('--save_estimates', type=str2bool, default=True)
  a('--save_corresp', type=str2bool, default=False)
  a('--infer_name', default=None)
  a('--fitting_method', default='progressive_x')
  a('--inlier_thresh', type=float, default=4.0)
  a('--neighbour_max_dist', type=float, default=20.0)
  a('--min_hypothesis_quality', type=float, default=0.5)
  a('--required_progx_confidence', type=float, default=0.5)
  a('--required_ransac_confidence', type=float, default=1.0)
  a('--min_triangle_area', type=float, default=0.0)
  a('--use_prosac', type=str2bool, default=False)
  a('--max_model_number_for_pearl', type=int, default=5)
  a('--spatial_coherence_weight', type=float, default=0.1)
  a('--scaling_from_millimeters', type=float, default=0.1)
  a('--max_tanimoto_similarity', type=float, default=0.9)
  a('--max_correspondences', type=int, default=None)
  a('--max_instances_to_fit', type=int, default=None)
  a('--detection_instance_cap', type=int, default=DETECTION_INSTANCE_CAP)   # not in the reference
  cli.add_precision_flags(ap)
  a('--max_fitting_iterations', type=int, default=400)
  a('--vis', type=str2bool, default=False)
  a('--vis_gt_poses', type=str2bool, default=True)           # infer.py:126-146
  a('--vis_pred_poses', type=str2bool, default=True)
  a('--vis_gt_obj_labels', type=str2bool, default=True)
  a('--vis_pred_obj_labels', type=str2bool, default=True)
  a('--vis_pred_obj_confs', type=str2bool, default=False)
  a('--vis_gt_frag_fields', type=str2bool, default=False)
  a('--vis_pred_frag_fields', type=str2bool, default=False)
  a('--vis_renderer', choices=('splat', 'mesh'), default='splat',
    help='not in the reference. splat (default): pose overlays as a z-buffered point splat '
         'on the host; no ground-truth label tile, no ground-truth fragment fields. mesh: the '
         'object meshes are rendered on the device (epos_amd/render.py; needs --dataset and '
         '$BOP_PATH for the \'eval\' models): shaded pose overlays, the "gt obj labels" tile '
         'and --vis_gt_frag_fields for frames that carry gt_poses')
  cli.add_dataset_flags(ap)
  a('--min_visib_fract', type=float, default=0.1)
  a('--corr_min_obj_conf', type=float, default=0.1)
  a('--corr_min_frag_rel_conf', type=float, default=0.5)
  a('--corr_project_to_model', type=str2bool, default=False,
    help='accepted and ignored, as in the reference: common.py:78-80 defines the flag and '
         'nothing reads it (the projection switch that acts is --project_to_surface)')
  cli.add_network_flags(ap)
  cli.add_input_flags(ap)
  a('--batch', type=int, default=1, help='images per GPU per step')
  a('--seed', type=int, default=0)
  a('--pipeline_depth', type=int, default=0,
    help='batches in flight (independent plans on their own HIP streams, each with its own '
         'per-stage timers). 0 (default) = bench.py\'s rule: 4 at one image per batch, 2 from '
         'four images per batch on, 3 in between; 1 = strictly one batch at a time (the '
         'reference\'s loop). --vis, --save_corresp and the operator path '
         '(--project_to_surface, --order_on_device=false) read the plan\'s buffers after every '
         'step and always run at depth 1. The poses do not depend on the depth.')
  a('--launch_queue', type=int, default=int(os.environ.get('EPOS_LAUNCH_QUEUE', '2')),
    help='batches enqueued per plan before the oldest is collected: with 2 a plan\'s next '
         'batch is already in its stream when the current one finishes (the stream does not wait '
         'for the host between two batches). 1 whenever --vis / --save_corresp / the operator '
         'path read the plan\'s buffers after a step. The poses do not depend on it.')
  a('--sparse_heads', default='auto',
    help='evaluate the fragment heads only for the target objects of each image. '
         'corresp.establish_many_to_many never reads the other objects\' channels in '
         'localization mode (corresp.py:39-43), so the poses are bit-identical and ~7 %% of the '
         'step is saved. auto (default) = on for --task_type=localization unless --vis, '
         '--save_corresp or the operator path need the dense prediction; true / false force it')
  a('--order_on_device', type=str2bool, default=True,
    help='true (default): --use_prosac / --max_correspondences order and cap the '
         'correspondences by confidence on the device, inside the fused pipeline (sparse '
         'heads, several steps in flight). false: the run goes operator by operator (network '
         '-> correspondences -> host sort -> one fitting call per object, one step at a time, '
         'dense heads) -- same poses, kept for A/B runs on one box.')
  a('--surface_on_device', type=str2bool, default=False,
    help='not in the reference. true: --project_to_surface runs inside the fused pipeline '
         '(closest points through a mesh index, on the device; sparse heads, several steps in '
         'flight) -- the same poses as the default, operator-by-operator route of that flag, '
         'which stays the default.')
  cli.add_decode_flags(ap)
  return ap


def fitting_path(use_prosac, max_correspondences, project_to_surface, order_on_device,
                 surface_on_device=False):
  """(operator_path, order_in_pipeline). operator_path: the run goes operator by operator
  (process_by_operators) instead of through the fused device pipeline -- for
  --project_to_surface unless --surface_on_device puts the mesh query into the pipeline, and
  whenever --order_on_device is false. order_in_pipeline: the fused pipeline gets the device-side
  confidence order (--use_prosac and/or --max_correspondences on the fused path)."""
  operator_path = (bool(project_to_surface) and not surface_on_device) or not order_on_device
  order_in_pipeline = not operator_path and (bool(use_prosac) or
                                             max_correspondences is not None)
  return operator_path, order_in_pipeline


def resolve_sparse_heads(args, needs_dense, pyramid):
  """--sparse_heads: auto = on for localization unless the dense heads are read (--vis,
  --save_corresp, the operator path) or an image pyramid is on (its merge reads every
  object's heads of every scale); true where that is not possible raises ValueError."""
  sh = str(args.sparse_heads).lower()
  if sh == 'auto':
    return args.task_type == pipeline.LOCALIZATION and not needs_dense and pyramid is None
  sparse_heads = cli.str2bool(sh)
  if sparse_heads and pyramid is not None:
    raise ValueError('--sparse_heads=true is not available with --image_pyramid '
                     '(multi-scale heads are dense).')
  if sparse_heads and (needs_dense or args.task_type != pipeline.LOCALIZATION):
    raise ValueError('--sparse_heads=true needs --task_type=localization without --vis / '
                     '--save_corresp / the operator path (they read every object\'s heads)')
  return sparse_heads


def save_correspondences(infer_dir, infer_name, frame, im_ind, corr, pred_time):
  """infer.py:294-345 text dump (sorted by confidence)."""
  scene_id, im_id, K = frame.scene_id, frame.im_id, frame.K
  for obj_id, c in corr.items():
    txt = '# Corr format: u v x y z px_id frag_id conf conf_obj conf_frag\n'
    txt += 'synthetic\n{} {} {} {}\n'.format(scene_id, im_id, obj_id, pred_time)
    for i in range(3):
      txt += '{} {} {}\n'.format(K[i, 0], K[i, 1], K[i, 2])
    txt += '0\n'
    order = np.argsort(c['conf'])[::-1]
    txt += '{}\n'.format(len(order))
    for i in order:
      txt += '{} {} {} {} {} {} {} {} {} {}\n'.format(
          c['coord_2d'][i, 0], c['coord_2d'][i, 1], c['coord_3d'][i, 0],
          c['coord_3d'][i, 1], c['coord_3d'][i, 2], c['px_id'][i],
          c['frag_id'][i], c['conf'][i], c['conf_obj'][i], c['conf_frag'][i])
    path = os.path.join(infer_dir, 'corr' + cli.result_suffix(infer_name),
                        '{:06d}_corr_{:02d}.txt'.format(im_ind, obj_id))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
      f.write(txt)


def process_by_operators(pipe, store, imgs, chunk, targets, args, fit):
  """process_image (infer.py:348-554) call by call: predict -> corresp ->
  [PROSAC sort / top-K by confidence, infer.py:425-440] -> find6DPoses per object."""
  from epos_amd import corresp as ecorresp
  t0 = time.time()
  pred = pipe.net.forward(imgs, use_graph=pipe.use_graph)
  torch.cuda.synchronize()
  t1 = time.time()
  poses = []
  t_corr = t_fit = 0.0
  for b, f in enumerate(chunk):
    tc = time.time()
    corr = ecorresp.establish_many_to_many(
        pred['pred_obj_conf'][b], pred['pred_frag_conf'][b],
        pred['pred_frag_loc'][b], list(targets[b]), store, pipe.output_scale,
        args.corr_min_obj_conf, args.corr_min_frag_rel_conf,
        bool(args.project_to_surface),
        args.task_type == pipeline.LOCALIZATION, device=str(pipe.dev))
    t_corr += time.time() - tc
    tf_ = time.time()
    for obj_id, c in corr.items():
      n = c['coord_2d'].shape[0]
      if n < 6:                                           # infer.py:420-422
        continue
      if args.use_prosac:                                 # infer.py:425-428
        order = ecorresp.confidence_order(c['conf'])
        c = {k: v[order] for k, v in c.items()}
      if args.max_correspondences is not None and n > args.max_correspondences:
        keep = (np.arange(n) if args.use_prosac else
                ecorresp.confidence_order(c['conf']))[:args.max_correspondences]
        c = {k: v[keep] for k, v in c.items()}           # infer.py:431-440
      num_inst = (targets[b].get(obj_id, 1)
                  if args.task_type == pipeline.LOCALIZATION else -1)
      if args.max_instances_to_fit is not None:
        num_inst = min(num_inst, args.max_instances_to_fit)
      if args.fitting_method == 'opencv_ransac':
        # infer.py:505-528: cv2.solvePnPRansac(EPNP) -- ONE instance per object, score 0.0.
        # OpenCV is not in this stack; epos_amd.fitting.solvePnPRansac runs the same
        # algorithm (5-point EPnP sets drawn by cv::RNG, float32 inlier rule, the 0.99
        # confidence bound, EPnP over the inliers) in HIP -- csrc/epnp_ransac.hip.
        # The pose is taken as the kernels computed it (return_pose), as the fused pipeline
        # reports it: R -> rvec -> Rodrigues(rvec) on the host (infer.py:526) moves R by an
        # ulp and would make the two routes differ in the last bit.
        ok, _, t_est, _, pose = fitting.solvePnPRansac(
            objectPoints=c['coord_3d'], imagePoints=c['coord_2d'], cameraMatrix=f.K,
            distCoeffs=None, iterationsCount=fit.max_iters,
            reprojectionError=fit.threshold, confidence=0.99,
            flags=fitting.SOLVEPNP_EPNP, return_pose=True)
        if ok:
          poses.append({'scene_id': f.scene_id, 'im_id': f.im_id, 'obj_id': obj_id,
                        'R': pose[:, :3].copy(), 't': t_est, 'score': 0.0})
        continue
      est, _, quals = fitting.find6DPoses(
          c['coord_2d'], c['coord_3d'], f.K, threshold=fit.threshold,
          neighborhood_ball_radius=fit.neighborhood_ball_radius,
          spatial_coherence_weight=fit.spatial_coherence_weight,
          scaling_from_millimeters=fit.scaling_from_millimeters,
          max_tanimoto_similarity=fit.max_tanimoto_similarity,
          max_iters=fit.max_iters, conf=fit.conf,
          proposal_engine_conf=fit.proposal_engine_conf,
          min_coverage=fit.min_coverage,
          min_triangle_area=fit.min_triangle_area, min_point_number=6,
          max_model_number=num_inst,
          max_model_number_for_optimization=fit.max_model_number_for_optimization,
          use_prosac=args.use_prosac,
          seed=args.seed * 1000003 + f.im_id * 1009 + obj_id)
      if est is not None:                                 # infer.py:490-503
        for i in range(est.shape[0] // 3):
          poses.append({'scene_id': f.scene_id, 'im_id': f.im_id, 'obj_id': obj_id,
                        'R': est[3 * i:3 * i + 3, :3],
                        't': est[3 * i:3 * i + 3, 3].reshape(3, 1),
                        'score': float(quals[i])})
    t_fit += time.time() - tf_
  rt = {'prediction': t1 - t0, 'establish_corr': t_corr, 'fitting': t_fit}
  rt['total'] = sum(rt.values())
  for p in poses:
    p['time'] = rt['total']
  return poses, rt


def prepare(argv=None):
  """Parses the command line, applies params.yml, refuses what this build cannot run and
  prints the notes. Returns (args, model_dir, (rank, world, local_rank))."""
  args = build_parser().parse_args(argv)
  ranks = edist.init_from_env()
  model_dir = cli.model_dir(args)
  cli.update_flags(args, os.path.join(model_dir, cli.PARAMS_FILENAME))  # infer.py:561-564
  cli.check_supported_flags(args)
  if args.cpu_only:
    raise SystemExit('--cpu_only: this build has no CPU path (MI355X only).')
  if args.fitting_method not in ('progressive_x', 'opencv_ransac'):
    raise ValueError('Unknown pose fitting method ({}).'.format(
        args.fitting_method))                                   # infer.py:530-532
  if args.fitting_method == 'opencv_ransac':
    # not bit-for-bit cv2 (which cannot be installed or checked here): say so at run time
    print('NOTE --fitting_method=opencv_ransac: the algorithm cv2.solvePnPRansac(EPNP) '
          'publishes (cv::RNG 5-point sets, EPnP, float32 inlier rule, the shrinking 0.99 '
          'bound with a once-rounded w^5, the float32 round trip of the normalised image '
          'points, EPnP over the inliers) runs in HIP, but its poses are NOT guaranteed to '
          'equal cv2\'s bit for bit: the factorisations are this build\'s own and the '
          'R -> rvec -> R round trip through cv::Rodrigues in front of the inlier test is '
          'not made (DESIGN.md (f2)).')
  mesh_vis = bool(args.vis) and args.vis_renderer == 'mesh'
  if mesh_vis and not (args.dataset and os.environ.get('BOP_PATH')):
    raise ValueError('--vis_renderer mesh needs --dataset and $BOP_PATH (object models)')
  if args.vis and args.vis_gt_frag_fields and not mesh_vis:
    raise NotImplementedError(
        '--vis_gt_frag_fields needs the ground-truth fragment fields of the training '
        'pipeline (datagen.py:478-544), which the inference reader does not build.')
  if args.vis and args.vis_gt_obj_labels and not mesh_vis:
    # the GT label map comes from the instance masks of the training reader
    # (datagen.py:478-544); the inference reader holds none, so that tile is left out --
    # said once here instead of silently (scripts/infer.py:150-291 draws it)
    print('note: --vis_gt_obj_labels has no ground-truth label map at inference; the tile '
          'is omitted (use --vis_gt_obj_labels=False to silence this)', file=sys.stderr)
  return args, model_dir, ranks


def build_pipelines(args, model_dir, ranks):
  """Everything the loop of main() runs on, as one namespace: the model store, this rank's
  frames, the fit parameters, the resolved depth / launch queue / heads, the renderer of
  --vis_renderer mesh, the prefetcher and the warmed-up pipelines."""
  rank, world, local_rank = ranks
  checkpoint_dir = os.path.join(model_dir, 'train')             # infer.py:570
  dev_index = cli.device_from_env(local_rank)
  dev = 'cuda:%d' % dev_index
  torch.cuda.set_device(dev_index)

  ckpt, num_objs, _ = cli.load_checkpoint(args, checkpoint_dir)
  store = cli.resolve_store(model_dir, args, num_objs, dev)
  frames, h, w = cli.load_frames(
      args.infer_tfrecord_names, args.frames, args.synthetic, args.infer_crop_size,
      args.infer_max_height_before_crop, args.seed, num_objs, rank, world,
      store.dp_model['obj_ids'])
  fit = fitting.fit_params(
      threshold=args.inlier_thresh,
      neighborhood_ball_radius=args.neighbour_max_dist,
      spatial_coherence_weight=args.spatial_coherence_weight,
      scaling_from_millimeters=args.scaling_from_millimeters,
      max_tanimoto_similarity=args.max_tanimoto_similarity,
      max_iters=args.max_fitting_iterations,
      conf=args.required_progx_confidence,
      proposal_engine_conf=args.required_ransac_confidence,
      min_coverage=args.min_hypothesis_quality,
      min_triangle_area=args.min_triangle_area, min_point_number=6,
      max_model_number_for_optimization=args.max_model_number_for_pearl,
      use_prosac=args.use_prosac)
  # max_correspondences / use_prosac (both off by default, infer.py:95-97,115-117) order and
  # cap the correspondences by confidence (infer.py:425-440): inside the fused pipeline, on
  # the device (pipeline.EposPipeline(max_correspondences=..., fit use_prosac)). Only
  # project_to_surface (off by default; it needs the object meshes) without
  # --surface_on_device=true, and --order_on_device=false, go operator by operator (HIP network
  # -> HIP correspondences -> host sort -> HIP fitting per object) instead. With
  # --surface_on_device=true the mesh query is a stage of the fused pipeline
  # (pipeline.EposPipeline(project_to_surface=True)) and the run resolves like a plain one.
  operator_path, order_in_pipeline = fitting_path(
      args.use_prosac, args.max_correspondences, args.project_to_surface,
      args.order_on_device, args.surface_on_device)
  if args.project_to_surface:
    # infer.py:622 prepare_for_projection: the 'eval' models of the dataset
    # (datagen.py:250-252,299-306), closest-point queries on the GPU
    from epos_amd import ply
    bop = os.environ.get('BOP_PATH')
    if not (args.dataset and bop):
      raise ValueError('--project_to_surface needs --dataset and $BOP_PATH (object models)')
    store.models = ply.load_models(bop, args.dataset, 'eval',
                                   obj_ids=store.dp_model['obj_ids'])
  renderer = frag_pool = None
  if args.vis and args.vis_renderer == 'mesh':
    # scripts/infer.py:633-638: the renderer holds the 'eval' models (those of
    # --project_to_surface when it loaded them already)
    from epos_amd import ply, render as erender
    renderer = cli.eval_renderer(getattr(store, 'models', None) or ply.load_models(
        os.environ['BOP_PATH'], args.dataset, 'eval', obj_ids=store.dp_model['obj_ids']), dev)
    frag_pool = erender.pool_fragments(store.frag_centers, store.frag_sizes)
  B = args.batch
  # Instances per object (infer.py:456-468 of the reference): localization fits as many as
  # the frame's annotations hold -- the plan is sized for the largest count among the frames
  # read, nothing is clamped; --max_instances_to_fit lowers the counts as in the reference
  # (scripts/infer.py:467-468). Detection ("all found", -1): the reference's
  # min(-1, max_instances_to_fit) stays -1, i.e. the flag does not act there; this build
  # bounds "all found" by --detection_instance_cap (static buffers) and reports every
  # (frame, object) that reaches the cap.
  if args.task_type == pipeline.LOCALIZATION:
    max_inst = max([1] + [int(c) for f in frames for c in f.targets.values()])
    if args.max_instances_to_fit is not None:
      max_inst = max(1, min(max_inst, args.max_instances_to_fit))
  else:
    max_inst = max(1, int(args.detection_instance_cap))
  needs_dense = bool(operator_path or args.save_corresp or args.vis)
  depth = args.pipeline_depth if args.pipeline_depth > 0 else (
      4 if B == 1 else 2 if B >= 4 else 3)         # bench.py's rule
  lq = max(1, args.launch_queue)
  if needs_dense:
    depth = 1                      # those paths read the plan's buffers after the step
    lq = 1
  if depth == 1:
    lq = 1                         # strictly one batch at a time means launch -> collect
  pyramid = multiscale.normalize_pyramid(cli.as_list(args.image_pyramid, float) or None)
  sparse_heads = resolve_sparse_heads(args, needs_dense, pyramid)
  # the decoder processes start (import numpy / PIL) while the plans are built; nothing is
  # decoded before the loop of main() asks for it
  from epos_amd import frames as eframes
  mo = cli.model_options(args, num_objs, w, h, pyramid)
  feed = eframes.Prefetcher(frames, B, h, w, workers=args.decode_threads or None,
                            ahead=max(1, args.prefetch), inflight=depth * lq)
  pipes = [pipeline.EposPipeline(
      ckpt, B, h, w, num_objs, args.num_frags, store, fit_params=fit,
      corr_min_obj_conf=args.corr_min_obj_conf,
      corr_min_frag_rel_conf=args.corr_min_frag_rel_conf,
      max_instances=max_inst, model_options=mo, device=dev, instance=j,
      sparse_heads=sparse_heads, fitting_method=args.fitting_method, queue=lq,
      precision=args.precision, image_pyramid=pyramid,
      merge_method=args.merge_method if pyramid is not None else None,
      max_correspondences=args.max_correspondences if order_in_pipeline else None,
      project_to_surface=bool(args.project_to_surface) and not operator_path)
           for j in range(depth)]
  pipe = pipes[0]
  if rank == 0 and pyramid is not None:
    print('plan: image pyramid %s, merge %s, merged heads %dx%d' % (
        pyramid, args.merge_method, pipe.net.out_h, pipe.net.out_w))
    if max(pyramid) > 1.0:
      print('NOTE --image_pyramid with a scale above 1: the correspondences use the merged '
            'heads\' stride, output_scale = %g / 4; the reference passes 1/4 whatever the '
            'pyramid (scripts/infer.py:586-591,721) and would misplace them by a factor %g '
            '(DESIGN.md, "multi-scale mode").' % (max(pyramid), max(pyramid)))
  if rank == 0:
    print('plan: {} image(s) per step, {} step(s) in flight{}, {} heads, {} GEMM layers on the '
          'fp16-pair kernel ({} on the bf16 x 6 fallback)'.format(
              B, depth, ' x {} enqueued per plan'.format(lq) if lq > 1 else '',
              'sparse' if sparse_heads else 'dense', len(pipe.net.h2_layers),
              len(pipe.net.h2_refused)))

  # Set-up, not inference: every plan captures its hipGraph and loads its kernels on first
  # use, so each one runs once on a blank frame here (results discarded) -- the reference
  # likewise treats its first sess.run as warm-up (scripts/infer.py:741-749 replaces the first
  # image's time by the mean of the others).
  if frames and not operator_path:
    blank = torch.zeros((B, h, w, 3), dtype=torch.uint8).pin_memory()
    f0 = frames[0]
    tg0 = [dict(f0.targets)] * B
    if args.max_instances_to_fit is not None:
      tg0 = [{o: min(c, args.max_instances_to_fit) for o, c in t.items()} for t in tg0]
    for q in pipes:
      q.process_batch(blank, np.stack([f0.K] * B), tg0, task_type=args.task_type, seed=args.seed)
      q.cap_hits = collections.deque(maxlen=q.CAP_HITS_KEPT)
      q.last_cap_hits, q.cap_hit_count = [], 0
      q._warned_cap = False
    torch.cuda.synchronize()
  return types.SimpleNamespace(
      dev=dev, store=store, frames=frames, h=h, w=w, fit=fit, operator_path=operator_path,
      renderer=renderer, frag_pool=frag_pool, max_inst=max_inst, depth=depth, lq=lq, feed=feed,
      pipes=pipes)


def save_step_correspondences(args, run, infer_dir, i0, chunk, pred_time):
  """--save_corresp: the correspondences of the step's frames, from the dense heads the plan
  still holds."""
  from epos_amd import corresp as ecorresp
  pipe = run.pipes[0]
  pred = pipe.net.outputs()
  for b, f in enumerate(chunk):
    c = ecorresp.establish_many_to_many(
        pred['pred_obj_conf'][b], pred['pred_frag_conf'][b],
        pred['pred_frag_loc'][b], list(f.targets), run.store, pipe.output_scale,
        args.corr_min_obj_conf, args.corr_min_frag_rel_conf, False,
        args.task_type == pipeline.LOCALIZATION, device=run.dev)
    save_correspondences(infer_dir, args.infer_name, f, i0 + b, c, pred_time)


def visualize_step(args, run, model_dir, i0, chunk, poses):
  """--vis (infer.py:540-552): one image per frame of the step in <model>/vis (:577)."""
  from epos_amd import vis as evis
  pred = {k: v.cpu().numpy() for k, v in run.pipes[0].net.outputs().items()}
  flags = {k: getattr(args, k) for k in vars(args) if k.startswith('vis_')}
  for b, f in enumerate(chunk):
    est = [p for p in poses if (p['scene_id'], p['im_id']) == (f.scene_id, f.im_id)]
    gt_fields = None
    if run.renderer is not None:
      # the ground-truth maps at the output resolution, with output_K of datagen.py:482-488;
      # frames without instance masks (--frames, --synthetic) take the depth rule
      oh, ow = pred['pred_obj_label'][b].shape
      gt_fields = eval_utils.gt_fields_device(
          run.renderer, f, (ow, oh), run.frag_pool, lambda o: o in run.store.frag_centers,
          input_size=(run.w, run.h), allow_empty=False)
      if gt_fields is not None:
        gt_fields = {k: v.cpu().numpy() for k, v in gt_fields.items()}
    evis.visualize(f.image_f32(), f.K, {k: v[b] for k, v in pred.items()}, est, i0 + b,
                   run.store, os.path.join(model_dir, 'vis'),
                   gt_poses=f.gt_poses, flags=flags, renderer=run.renderer,
                   gt_fields=gt_fields)


def write_results(args, run, ranks, infer_dir, poses_all, time_start, loop_s, host_s):
  """After the loop: the cap-hit report, the first image's time, the gather over the ranks,
  the CSV and the throughput lines."""
  rank, world, _ = ranks
  frames, pipes = run.frames, run.pipes
  hits = sorted(set(h for q in pipes for h in q.cap_hits))
  n_hits = sum(q.cap_hit_count for q in pipes)
  if hits:
    overflowed = any(q.cap_hit_count > q.CAP_HITS_KEPT for q in pipes)
    print('Instance cap (--detection_instance_cap={}) reached {} time(s), for {} distinct '
          '(scene, image, object) triples{}; more instances may exist there:'.format(
              run.max_inst, n_hits, len(hits),
              ' among the last {} hits kept per pipeline'.format(pipes[0].CAP_HITS_KEPT)
              if overflowed else ''))
    for sc_, im_, ob_, n_ in hits:
      print('  scene {} image {} object {}: {} instances'.format(sc_, im_, ob_, n_))
  # First-image time := mean time of the others (infer.py:741-749).
  if len(poses_all) > 1 and frames:
    first = (frames[0].scene_id, frames[0].im_id)
    rest = [p['time'] for p in poses_all if (p['scene_id'], p['im_id']) != first]
    if rest:
      for p in poses_all:
        if (p['scene_id'], p['im_id']) == first:
          p['time'] = float(np.mean(rest))
  # max_records=None: the ranks first agree on the largest local pose count (their
  # shards differ by a frame whenever N % world != 0, and a rank may hold none)
  merged = edist.gather_poses(poses_all, max_records=None) if world > 1 else poses_all
  if rank == 0 and args.save_estimates:
    path = os.path.join(infer_dir, 'estimated-poses{}.csv'.format(
        cli.result_suffix(args.infer_name)))
    bop_io.save_bop_results(path, merged, version='bop19')
    total_s = time.time() - time_start
    print('Saved {} pose estimates to: {}  ({:.2f} s)'.format(len(merged), path, total_s))
    # from the first decode to the CSV on disk (this rank's frames; with N ranks each rank
    # runs its own shard concurrently, so the job's rate is ~N x this)
    print('Throughput: {} images in {:.3f} s = {:.1f} images/s (inference loop {:.3f} s = '
          '{:.1f} images/s; first decode -> CSV written; plan construction and weight packing '
          'before it are not included)'.format(
              len(frames), total_s, len(frames) / max(total_s, 1e-9), loop_s,
              len(frames) / max(loop_s, 1e-9)))
    if not run.operator_path:
      n_steps = max(1, (len(frames) + args.batch - 1) // args.batch)
      print('Host time per step [ms]: ' + ', '.join(
          '{} {:.3f}'.format(k, v / n_steps * 1e3) for k, v in host_s.items()))


def main(argv=None):
  args, model_dir, ranks = prepare(argv)
  rank, world, _ = ranks
  infer_dir = os.path.join(model_dir, 'infer')
  os.makedirs(infer_dir, exist_ok=True)
  run = build_pipelines(args, model_dir, ranks)
  frames, feed, pipes, B = run.frames, run.feed, run.pipes, args.batch
  depth, lq = run.depth, run.lq

  poses_all = []
  time_start = time.time()           # first decode -> CSV written

  def finish(i0, chunk, poses, rt):
    n_real = len(frames[i0:i0 + B])
    real_ids = set((f.scene_id, f.im_id) for f in frames[i0:i0 + n_real])
    seen = set()
    for p in poses:
      p.setdefault('time', rt.get('total', 0.0))
      key = (p['scene_id'], p['im_id'], p['obj_id'], float(p['score']))
      if (p['scene_id'], p['im_id']) in real_ids and key not in seen:
        seen.add(key)
        poses_all.append(p)
    if args.save_corresp:
      save_step_correspondences(args, run, infer_dir, i0, chunk[:n_real], rt.get('total', 0.0))
    if args.vis:
      visualize_step(args, run, model_dir, i0, chunk[:n_real], poses)
    if rank == 0:                               # infer.py:730-734
      print('Image: {}, prediction: {:.3f}, establish_corr: {:.3f}, fitting: '
            '{:.3f}, total time: {:.3f}'.format(
                i0, rt.get('prediction', 0), rt.get('establish_corr', 0),
                rt.get('fitting', 0), rt.get('total', 0)))
    feed.release(i0)                            # its staging buffer may be decoded into again

  inflight = []                                 # (pipeline, i0, chunk), oldest first
  # HIP events around the stages (the per-image times the reference prints, infer.py:730-734);
  # EPOS_INFER_TIMING=0 runs without them (diagnostics: tools/infer_diag.sh)
  stage_timing = os.environ.get('EPOS_INFER_TIMING', '1') != '0'
  # where the host's time goes, per loop phase (printed with the throughput line): waiting for
  # decoded frames, waiting for the oldest step in flight, enqueueing a step, bookkeeping
  host_s = {'wait_frames': 0.0, 'wait_gpu': 0.0, 'launch': 0.0, 'finish': 0.0}
  clock = time.perf_counter
  t_mark = clock()
  for step, (i0, chunk, imgs) in enumerate(feed):
    # imgs: pinned host memory, uint8 as decoded (float32 only for frames that are not
    # byte-valued); the upload is enqueued on the step's own stream and the cast to float32
    # (datagen.py:435-436) runs on the device
    t_now = clock(); host_s['wait_frames'] += t_now - t_mark; t_mark = t_now
    Ks = np.stack([f.K for f in chunk])
    tg = [f.targets for f in chunk]
    if args.max_instances_to_fit is not None:  # infer.py:467-468
      tg = [{o: min(c, args.max_instances_to_fit) for o, c in t.items()}
            for t in tg]
    if run.operator_path:
      poses, rt = process_by_operators(pipes[0], run.store, imgs, chunk, tg, args, run.fit)
      finish(i0, chunk, poses, rt)
      t_mark = clock()
      continue
    if len(inflight) == depth * lq:
      q, j0, ch = inflight.pop(0)
      res = q.collect()
      t_now = clock(); host_s['wait_gpu'] += t_now - t_mark; t_mark = t_now
      finish(j0, ch, *res)
      t_now = clock(); host_s['finish'] += t_now - t_mark; t_mark = t_now
    p = pipes[step % depth]
    p.launch(imgs, Ks, tg, task_type=args.task_type,
             image_ids=[f.im_id for f in chunk], scene_ids=[f.scene_id for f in chunk],
             seed=args.seed, timing=stage_timing)
    inflight.append((p, i0, chunk))
    t_now = clock(); host_s['launch'] += t_now - t_mark; t_mark = t_now
  while inflight:
    q, j0, ch = inflight.pop(0)
    res = q.collect()
    t_now = clock(); host_s['wait_gpu'] += t_now - t_mark; t_mark = t_now
    finish(j0, ch, *res)
    t_now = clock(); host_s['finish'] += t_now - t_mark; t_mark = t_now
  loop_s = time.time() - time_start
  write_results(args, run, ranks, infer_dir, poses_all, time_start, loop_s, host_s)
  if world > 1:
    torch.distributed.destroy_process_group()


if __name__ == '__main__':
  main()
