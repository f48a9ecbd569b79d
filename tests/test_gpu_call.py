"""epos_amd/_call.py on the device: the stream a wrapper hands to the C entry is the current
stream of the tensor's device, here a side stream."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import heads_wgrad_ref as ref          # noqa: E402

pytestmark = pytest.mark.gpu


def test_launch_takes_the_side_stream_and_the_kernel_runs_on_it():
  from epos_amd import _call, heads_train
  dev = torch.device('cuda:0')
  rng = np.random.RandomState(7)
  w, a, g = (rng.randn(64).astype(np.float32) for _ in range(3))
  side = torch.cuda.Stream(dev)
  assert side.cuda_stream != torch.cuda.current_stream(dev).cuda_stream
  with torch.cuda.stream(side):
    with _call.launch(dev) as q:
      assert q.handle.value == side.cuda_stream and q.stream == side
    assert _call.stream_handle(dev)[1].value == side.cuda_stream
    dw, da, dg = (torch.from_numpy(x).to(dev, non_blocking=True) for x in (w, a, g))
    heads_train.momentum_step(dw, da, dg, 0.01, 0.9, 4e-5, 2.0)
  side.synchronize()                # the side stream alone: uploads and kernel were enqueued on it
  w2, a2 = ref.momentum_step(w, a, g, 0.01, 0.9, 4e-5, 2.0)
  assert dw.cpu().numpy().tobytes() == w2.tobytes()
  assert da.cpu().numpy().tobytes() == a2.tobytes()
  assert torch.equal(dg.cpu(), torch.from_numpy(g))
