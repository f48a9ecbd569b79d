#!/usr/bin/env python
"""Times the five loss / gradient entries with k = 1, 2, 4 nearest fragments per pixel
(include/epos_hip.h, "k nearest fragments") at C2's sizes -- 120 x 160 heads, 21 objects x 64
fragments, K = 256 features, B = 1 and 8 -- and, at k = 1, the entries of a library built from
the PARENT commit next to this build's, in the same process, window after window in turn.

    python tools/bench_knn.py --build-parent [--parent-rev HEAD~1]   # where git and hipcc are
    python tools/bench_knn.py [--out profiles/r29] [--train-step]    # on the MI355X

--build-parent compiles the sources of --parent-rev (git archive) into
epos_amd/lib/libepos_hip_parent.so and a second copy, libepos_hip_parent2.so: two handles of the
same code, so that parent-against-parent is measured exactly as parent-against-this is.

What is written (bench_knn.json and bench_knn.md under --out):
  * per entry, B and build: the median and the range over WINDOWS windows of the time per call,
    each window REPS calls between two device events, REPS sized so that a window lasts about
    WINDOW_MS; every build's windows alternate with the others';
  * at k = 1, this build's old entry and its _knn entry over the parent's, and parent2 / parent
    (the spread); the _knn entry passes one argument more through ctypes, which shows in the
    entries whose windows are bound by the rate of launches;
  * a sha256 of every output (all its bytes) of the parent build, of this build's old entries
    and of this build's _knn entries at k = 1, on the same seeded inputs: they must be equal;
  * with --train-step: trainer.train_step at 640 x 480, B = 1, k = 1, 2, 4 (this build only:
    the Python layer calls the _knn entries, which the parent library does not have).
"""
import argparse
import ctypes
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

H, W, O, F, K = 120, 160, 21, 64, 256
P = H * W
WINDOWS, WINDOW_MS, WARMUP = 9, 100.0, 5
IGNORE = 255
HASH_BYTES = 1 << 28
ENTRIES = ('epos_loss_terms', 'epos_loss_reduce', 'epos_loss_grads', 'epos_heads_wgrad_f32',
           'epos_heads_dgrad_f32')
KNN_NAME = {'epos_loss_terms': 'epos_loss_terms_knn', 'epos_loss_reduce': 'epos_loss_reduce_knn',
            'epos_loss_grads': 'epos_loss_grads_knn',
            'epos_heads_wgrad_f32': 'epos_heads_wgrad_knn_f32',
            'epos_heads_dgrad_f32': 'epos_heads_dgrad_knn_f32'}
KNN_AT = {'epos_loss_terms': 13, 'epos_loss_reduce': 8, 'epos_loss_grads': 13,
          'epos_heads_wgrad_f32': 16, 'epos_heads_dgrad_f32': 13}     # where `int knn` goes


def parent_paths():
  from epos_amd import build
  return (os.path.join(build.LIB_DIR, 'libepos_hip_parent.so'),
          os.path.join(build.LIB_DIR, 'libepos_hip_parent2.so'))


def build_parent(rev):
  from epos_amd import build
  out, out2 = parent_paths()
  os.makedirs(build.LIB_DIR, exist_ok=True)
  tmp = tempfile.mkdtemp(prefix='epos_parent_')
  try:
    tar = subprocess.run(['git', '-C', ROOT, 'archive', rev, 'epos_amd/csrc', 'include'],
                         check=True, capture_output=True).stdout
    subprocess.run(['tar', '-x', '-C', tmp], input=tar, check=True)
    srcs = sorted(os.path.join(tmp, 'epos_amd', 'csrc', f)
                  for f in os.listdir(os.path.join(tmp, 'epos_amd', 'csrc')) if f.endswith('.hip'))
    subprocess.check_call([build.HIPCC] + build.FLAGS + ['-Wno-inline-asm', '-o', out] + srcs)
  finally:
    shutil.rmtree(tmp, ignore_errors=True)
  shutil.copyfile(out, out2)
  print('built %s (and its copy) from %s' % (out, rev))


def open_parent(path):
  """The parent library's old entries, bound with the argument types of _lib.SYMBOLS."""
  from epos_amd import _lib
  lib = ctypes.CDLL(path)
  for name in ENTRIES + ('epos_loss_workspace_bytes', 'epos_heads_wgrad_workspace_bytes'):
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _lib.SYMBOLS[name]
  return lib


def make_inputs(B, knn, seed):
  """Seeded logits, features, weights and a ground truth with about a third of the pixels in
  the foreground and knn different fragments per foreground pixel, on the device."""
  import torch
  g = torch.Generator(device='cuda')
  g.manual_seed(seed)
  n = B * P

  def randn(*shape, scale=1.0):
    return torch.randn(shape, generator=g, device='cuda', dtype=torch.float32) * scale
  t = {'obj': randn(n, O + 1, scale=4.0), 'frag': randn(n, O, F, scale=4.0),
       'loc': randn(n, O, F, 3, scale=1.5), 'A': torch.relu(randn(n, K, scale=1.5)),
       'wt': [randn(m, K, scale=0.1) for m in (O + 1, O * F, O * F * 3)]}
  # runs of eight pixels of one label, two thirds of them background
  runs = torch.randint(0, 3 * (O + 1), (B, P // 8), generator=g, device='cuda')
  runs = torch.where(runs > O, torch.zeros_like(runs), runs)
  t['g_obj'] = runs.repeat_interleave(8, dim=1).to(torch.int32).contiguous()
  order = torch.rand((n, F), generator=g, device='cuda').argsort(dim=1)
  t['g_frag'] = order[:, :knn].to(torch.int32).contiguous()
  t['g_loc'] = randn(n, knn, 3, scale=1.5)
  t['g_w'] = torch.rand((n, knn), generator=g, device='cuda') * 1.75 + 0.25
  return t


class Calls(object):
  """The five entries of one library over one set of inputs, outputs allocated once. knn None:
  the old entries."""

  def __init__(self, lib, t, B, knn, ws_lib=None):
    import torch
    self.lib, self.t, self.B, self.knn = lib, t, B, knn
    ws_lib = ws_lib or lib
    n = B * P
    f64, i64, f32 = torch.float64, torch.int64, torch.float32

    def new(shape, dtype):
      return torch.empty(shape, dtype=dtype, device='cuda')
    self.ws_loss = new((ws_lib.epos_loss_workspace_bytes(B, P, O, F) // 8,), i64)
    self.ws_wgrad = new((ws_lib.epos_heads_wgrad_workspace_bytes(B, P, O, F, K) // 8 + 1,), i64)
    self.out = {'sums': new((B, O + 1, 3), f64), 'counts': new((B, O + 1, 2), i64),
                'bad': new((B,), i64), 'values': new((4,), f64), 'scales': new((B, 3), f64),
                'd_obj': new((n, O + 1), f32), 'd_frag': new((n, O, F), f32),
                'd_loc': new((n, O, F, 3), f32), 'dX': new((n, K), f32)}
    for h, m in (('obj', O + 1), ('frag', O * F), ('loc', O * F * 3)):
      self.out['dW_' + h], self.out['db_' + h] = new((K, m), f32), new((m,), f32)

  def call(self, entry):
    import torch
    p = lambda x: ctypes.c_void_p(x.data_ptr())                           # noqa: E731
    t, o, B = self.t, self.out, self.B
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = [p(t['obj']), O + 1, p(t['frag']), p(t['loc']), p(t['g_obj']), p(t['g_frag']),
            p(t['g_loc']), p(t['g_w']), B, P, O, F, IGNORE]
    if entry == 'epos_loss_terms':
      args = head + [p(self.ws_loss), p(o['sums']), p(o['counts']), p(o['bad']), stream]
    elif entry == 'epos_loss_reduce':
      args = [p(o['sums']), p(o['counts']), B, O, 1.0, 1.0, 100.0, 1, p(o['values']),
              p(o['scales']), stream]
    elif entry == 'epos_loss_grads':
      args = head + [p(o['scales']), None, p(o['d_obj']), O + 1, p(o['d_frag']), p(o['d_loc']),
                     stream]
    elif entry == 'epos_heads_wgrad_f32':
      args = [p(t['A']), K, K] + head + [p(o['scales']), None, p(self.ws_wgrad)] + [
          p(o[k + h]) for h in ('obj', 'frag', 'loc') for k in ('dW_', 'db_')] + [stream]
    else:
      args = head + [p(o['scales']), None] + [p(w) for w in t['wt']] + [
          K, K, None, K, p(o['dX']), K, stream]
    name = entry
    if self.knn is not None:
      name = KNN_NAME[entry]
      args.insert(KNN_AT[entry], self.knn)
    rc = getattr(self.lib, name)(*args)
    if rc != 0:
      raise RuntimeError('%s returned %d' % (name, rc))

  def hashes(self):
    """sha256 of every output after one pass over the five entries in order. An output above
    HASH_BYTES is hashed in pieces of that size on the device's side of the copy: the digest
    is that of the whole tensor's bytes in order."""
    import torch
    for entry in ENTRIES:
      self.call(entry)
    torch.cuda.synchronize()
    out = {}
    for k, v in sorted(self.out.items()):
      h = hashlib.sha256()
      flat = v.view(-1).view(torch.uint8)
      for i in range(0, flat.numel(), HASH_BYTES):
        h.update(flat[i:i + HASH_BYTES].cpu().numpy().tobytes())
      out[k] = h.hexdigest()
    return out


def window(calls, entry, reps):
  import torch
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(reps):
    calls.call(entry)
  b.record()
  b.synchronize()
  return a.elapsed_time(b) / reps


def median(xs):
  s = sorted(xs)
  return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def time_entries(builds):
  """builds: [(label, Calls)]. Per entry the builds' windows alternate. Returns
  {entry: {label: [ms per call, per window]}}."""
  res = {}
  for entry in ENTRIES:
    for _, c in builds:                                  # the inputs of the later entries
      for e in ENTRIES[:ENTRIES.index(entry)]:
        c.call(e)
    reps = {}
    for label, c in builds:
      for _ in range(WARMUP):
        c.call(entry)
      reps[label] = max(5, int(WINDOW_MS / max(window(c, entry, 10), 1e-4)))
    res[entry] = {label: [] for label, _ in builds}
    for _ in range(WINDOWS):
      for label, c in builds:
        res[entry][label].append(window(c, entry, reps[label]))
  return res


def time_train_step(knns):
  import numpy as np
  import torch
  from epos_amd import model, synthetic, trainer, weights
  ckpt = weights.random_init('xception_65', num_objs=O, num_frags=F, seed=0, randomize_bn=True)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(O, F), crop_size=(4 * W, 4 * H))
  net = model.get_net(ckpt, 1, 4 * H, 4 * W, O, F, mo, 'cuda:0')
  img = torch.from_numpy(synthetic.image(0, 4 * H, 4 * W).astype(np.uint8)[None])
  opt = trainer.Optimizer(ckpt, 1e-6, momentum=0.9, weight_decay=4e-5)
  out = {}
  gts = {}
  for knn in knns:
    t = make_inputs(1, knn, seed=knn)
    slots = () if knn == 1 else (knn,)
    gts[knn] = {'obj_label': t['g_obj'].view(1, H, W),
                'frag_label': t['g_frag'].view((1, H, W) + slots),
                'frag_loc': t['g_loc'].view((1, H, W) + slots + (3,)),
                'frag_weight': t['g_w'].view((1, H, W) + slots)}
    for _ in range(3):
      trainer.train_step(net, img, gts[knn], opt, 1e-6)
    out[knn] = []
  torch.cuda.synchronize()
  for _ in range(WINDOWS):
    for knn in knns:
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      for _ in range(20):
        trainer.train_step(net, img, gts[knn], opt, 1e-6)
      b.record()
      b.synchronize()
      out[knn].append(a.elapsed_time(b) / 20)
  return out


def fmt(xs):
  return '%.4f (%.4f .. %.4f)' % (median(xs), min(xs), max(xs))


def main():
  ap = argparse.ArgumentParser(description=__doc__,
                               formatter_class=argparse.RawTextHelpFormatter)
  ap.add_argument('--build-parent', action='store_true')
  ap.add_argument('--parent-rev', default='HEAD~1')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r29'))
  ap.add_argument('--train-step', action='store_true')
  args = ap.parse_args()
  if args.build_parent:
    build_parent(args.parent_rev)
    return
  import torch
  from epos_amd import _lib
  if not torch.cuda.is_available():
    raise SystemExit('bench_knn.py needs an MI355X: nothing is measured without one')
  this = _lib.load()
  parents = [open_parent(path) for path in parent_paths()]
  doc = {'sizes': {'h': H, 'w': W, 'O': O, 'F': F, 'K': K}, 'windows': WINDOWS,
         'window_ms': WINDOW_MS, 'entries': {}, 'hashes': {}}
  lines = ['# k nearest fragments: the five entries at C2\'s sizes', '',
           'ms per call: median (min .. max) over %d windows of about %d ms, the builds\' windows '
           'in turn. parent2 is a second copy of the parent library: parent2 / parent is the '
           'spread of the measurement. "this, old entry" is this build\'s epos_* entry without '
           'knn, "this k=1" its _knn sibling.' % (WINDOWS, WINDOW_MS), '']
  for B in (1, 8):
    t1 = make_inputs(B, 1, seed=100 + B)
    builds = [('parent', Calls(parents[0], t1, B, None)), ('this old', Calls(this, t1, B, None)),
              ('this k=1', Calls(this, t1, B, 1)), ('parent2', Calls(parents[1], t1, B, None))]
    hashes = {'parent': builds[0][1].hashes(), 'this, old entries': builds[1][1].hashes(),
              'this, _knn entries at k=1': builds[2][1].hashes()}
    equal = len(set(json.dumps(h, sort_keys=True) for h in hashes.values())) == 1
    doc['hashes']['B=%d' % B] = dict(hashes, equal=equal)
    for knn in (2, 4):
      builds.append(('this k=%d' % knn, Calls(this, make_inputs(B, knn, seed=100 + B), B, knn)))
    res = time_entries(builds)
    doc['entries']['B=%d' % B] = res
    lines += ['## B = %d' % B, '', 'outputs of the three k = 1 routes: sha256 %s' % (
        'EQUAL, all %d tensors' % len(hashes['parent']) if equal else 'DIFFERENT'), '',
              '| entry | parent | this, old entry | this k=1 | old / parent | k=1 / parent | '
              'parent2 / parent | this k=2 | this k=4 |', '|---|---|---|---|---|---|---|---|---|']
    for entry in ENTRIES:
      r = res[entry]
      lines.append('| %s | %s | %s | %s | %.3f | %.3f | %.3f | %s | %s |' % (
          entry, fmt(r['parent']), fmt(r['this old']), fmt(r['this k=1']),
          median(r['this old']) / median(r['parent']),
          median(r['this k=1']) / median(r['parent']),
          median(r['parent2']) / median(r['parent']), fmt(r['this k=2']), fmt(r['this k=4'])))
    lines.append('')
    del builds, res
    torch.cuda.empty_cache()
  if args.train_step:
    ts = time_train_step((1, 2, 4))
    doc['train_step'] = {'k=%d' % k: v for k, v in ts.items()}
    lines += ['## trainer.train_step, 640 x 480, B = 1 (this build)', '', '| k | ms per step |',
              '|---|---|'] + ['| %d | %s |' % (k, fmt(v)) for k, v in ts.items()] + ['']
  os.makedirs(args.out, exist_ok=True)
  with open(os.path.join(args.out, 'bench_knn.json'), 'w') as f:
    json.dump(doc, f, indent=1, sort_keys=True)
  with open(os.path.join(args.out, 'bench_knn.md'), 'w') as f:
    f.write('\n'.join(lines))
  print('\n'.join(lines))
  if not all(v['equal'] for v in doc['hashes'].values()):
    raise SystemExit('the k = 1 outputs differ between the builds')


if __name__ == '__main__':
  main()
