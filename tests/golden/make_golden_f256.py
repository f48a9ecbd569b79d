#!/usr/bin/env python
"""Generates the f256_* golden fixtures under tests/golden/ from the REAL reference: the
correspondence and fragmentation cases of make_golden.py at more than 64 fragments per
object (the reference's "-f256" models; num_frags is an ordinary flag there).

Run in the build container only (needs the reference checkout make_golden.py imports):

    python tests/golden/make_golden_f256.py

Same stubbing and the same synthetic inputs as make_golden.py (whose helpers it imports);
the files carry the prefix f256_ so that the corresp_*.npz / fragment_*.npz globs of the
F = 64 tests do not collect them. The fixtures are data; no reference source travels.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G   # noqa: E402


def boundary_ties(obj, frag):
  """Exact ties at conf == max * tau_b (tau_b = 0.5) for object 1 on fragments that
  straddle the 64-bit mask words: a strict '>' drops the tied ones (corresp.py:64)."""
  F = frag.shape[3]
  tie, keep = 0.25, 0.25 + 2 ** -20
  for (y, x), tied, kept in (((1, 2), (63, 128, 191), (64, 127, 192, 255)),
                             ((2, 5), (64, 127, 192, 255), (0, 63, 128, 191))):
    obj[y, x, :] = 0.0
    obj[y, x, 1] = 1.0
    frag[y, x, 0, :] = 0.0
    frag[y, x, 0, 100] = 0.5                      # the maximum
    for f in tied:
      frag[y, x, 0, f] = tie                       # == 0.5 * 0.5 exactly: dropped
    for f in kept:
      frag[y, x, 0, f] = keep
  assert F == 256


def corresp_case(corresp, name, seed, h, w, num_objs, num_frags, gt_obj_ids,
                 only_annotated, sharp=2.0, modify=None, tau_a=0.1, tau_b=0.5,
                 output_scale=0.25):
  """make_golden.corresp_case with an optional in-place edit of the synthetic heads, written
  as f256_corresp_<name>.npz (the same fields)."""
  rng = np.random.RandomState(seed)
  obj, frag, loc = G.synth_heads(rng, h, w, num_objs, num_frags, sharp)
  if modify is not None:
    modify(obj, frag)
  centers, sizes = G.synth_store(rng, num_objs, num_frags)
  store = G.ModelStore(range(1, num_objs + 1), centers, sizes)
  out = corresp.establish_many_to_many(
      obj_confs=obj, frag_confs=frag, frag_coords=loc, gt_obj_ids=gt_obj_ids,
      model_store=store, output_scale=output_scale, min_obj_conf=tau_a,
      min_frag_rel_conf=tau_b, project_to_surface=False,
      only_annotated_objs=only_annotated)
  blob = {
      'obj_confs': obj, 'frag_confs': frag, 'frag_coords': loc,
      'gt_obj_ids': np.asarray(gt_obj_ids, np.int64),
      'only_annotated': np.asarray(only_annotated),
      'output_scale': np.asarray(output_scale, np.float64),
      'min_obj_conf': np.asarray(tau_a, np.float64),
      'min_frag_rel_conf': np.asarray(tau_b, np.float64),
      'frag_centers': np.stack([centers[o] for o in range(1, num_objs + 1)]),
      'frag_sizes': np.stack([sizes[o] for o in range(1, num_objs + 1)]),
      'out_obj_ids': np.asarray(sorted(out.keys()), np.int64),
  }
  for oid, d in out.items():
    for k, v in d.items():
      blob['out_%d_%s' % (oid, k)] = v
  path = os.path.join(HERE, 'f256_corresp_%s.npz' % name)
  np.savez_compressed(path, **blob)
  print(path, {o: len(d['px_id']) for o, d in out.items()})


def main():
  corresp, fragment = G.import_reference()
  # name, seed, h, w, O, F, gt ids, only_annotated (small maps: F = 256 is 4x the bytes;
  # every fixture stays below 1 MB)
  corresp_case(corresp, 'o3_s1', 1, 6, 10, 3, 256, [1, 3], True)
  corresp_case(corresp, 'o3_tie_s4', 4, 6, 8, 3, 256, [1, 2, 3], True,
               modify=boundary_ties)
  # Saturated: uniform confidences -> every pixel and every fragment kept.
  corresp_case(corresp, 'o3_full_s5', 5, 3, 4, 3, 256, [1, 2, 3], True, sharp=0.0)
  # No pixel above tau_a for any object -> empty dict (corresp.py:49).
  corresp_case(corresp, 'o3_empty_s7', 7, 3, 4, 3, 256, [1, 2, 3], True, sharp=0.0,
               tau_a=0.9)
  # Ragged size (not a multiple of 16 pixels) and a different scale.
  corresp_case(corresp, 'o2_ragged_s6', 6, 5, 7, 2, 256, [1, 2], True,
               output_scale=0.5, tau_a=0.3, tau_b=0.8)
  corresp_case(corresp, 'o21_s3', 3, 2, 4, 21, 256, [2, 5, 9, 14, 21], True, sharp=3.0)
  # F not a multiple of 64 (three mask words, the last one partial) and two full words.
  corresp_case(corresp, 'o3_f200_s8', 8, 6, 8, 3, 200, [1, 2, 3], True)
  corresp_case(corresp, 'o3_f128_s9', 9, 6, 8, 3, 128, [1, 2, 3], True, sharp=0.0)
  G.fragment_case(fragment, 'ellipsoid_f256_s2', 2, 3000, 256)
  os.replace(os.path.join(HERE, 'fragment_ellipsoid_f256_s2.npz'),
             os.path.join(HERE, 'f256_fragment_ellipsoid_s2.npz'))
  print('->', os.path.join(HERE, 'f256_fragment_ellipsoid_s2.npz'))


if __name__ == '__main__':
  main()
