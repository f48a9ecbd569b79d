"""Host time of the standalone weight update, this tree or the parent's (run from its root)."""
import os, sys, time, statistics as st
sys.path.insert(0, os.getcwd())
import torch
from epos_amd import net as enet, weights
try:
  from epos_amd import trainer
  opt_cls, name = trainer.Optimizer, 'set_weights'
except ImportError:
  from epos_amd import heads_train
  opt_cls, name = heads_train.HeadsOptimizer, 'set_head_weights'
H, W, O, F = 480, 640, 21, 64
ckpt = weights.random_init('xception_65', num_objs=O, num_frags=F, seed=0, randomize_bn=True)
net = enet.EposNet(ckpt, 1, H, W, O, F, device='cuda:0')
opt = opt_cls(ckpt, lr=1e-4)
net._build_sparse_packs()
fn = getattr(net, name)
for _ in range(30):
  fn(opt.params, check=False)
torch.cuda.synchronize()
host, dev = [], []
for _ in range(300):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  t0 = time.perf_counter()
  fn(opt.params, check=False)
  t1 = time.perf_counter()
  b.record()
  b.synchronize()
  host.append((t1 - t0) * 1e6)
  dev.append(a.elapsed_time(b) * 1e3)
q = lambda v: (st.median(v), min(v), sorted(v)[len(v) * 9 // 10])
print('%s: host us median %.1f min %.1f p90 %.1f; events us median %.1f min %.1f p90 %.1f' % (
    (name,) + q(host) + q(dev)))
