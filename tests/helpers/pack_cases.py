"""Shared by the weight-update tests: matrices for the device weight packer, the host packers'
bytes for a column window, and one grouped device call on numpy inputs."""
import ctypes

import numpy as np

# (K, N) of the issue; the last also as the window col0 = 64, N = 72 of a [256, 200] matrix
SIZES = [(4, 1), (8, 5), (16, 128), (20, 129), (256, 22), (256, 64), (256, 200)]
VALUE_SETS = ('normal', 'heavy_tailed', 'zero_column', 'subnormal', 'tiny', 'negative_zero')
FILL = 0xA5


def matrix(kind, K, N, seed):
  """(W f32 [K, N], bias f32 [N]) of one value set."""
  from epos_amd import weights
  rng = np.random.RandomState(seed)
  w = (0.05 * rng.standard_normal((K, N))).astype(np.float32)
  if kind == 'heavy_tailed':
    w = weights.heavy_tailed({'x/weights': w.reshape(1, 1, K, N)}, seed=seed)['x/weights']
    w = np.ascontiguousarray(w.reshape(K, N))
  elif kind == 'zero_column':
    w[:, N // 2] = 0.0
  elif kind == 'subnormal':                       # one fp32-subnormal weight beside normal ones
    w[K // 2, N // 2] = np.float32(1e-41)
    assert 0 < w[K // 2, N // 2] < np.finfo(np.float32).tiny
  elif kind == 'tiny':                            # 2^-30 of the column maximum: fp16-subnormal pieces
    w = (rng.standard_normal((K, N)) * 2.0 ** -30).astype(np.float32)
    w[0] = 1.0
  elif kind == 'negative_zero':
    w[K // 2, :] = -0.0
    w[0, N // 2] = -0.0
  else:
    assert kind == 'normal', kind
  return w, rng.standard_normal(N).astype(np.float32)


def problems(kind, seed=0):
  """The issue's eight problems of one value set: (W [K, ldw], bias [ldw], col0, N)."""
  out = []
  for i, (K, N) in enumerate(SIZES):
    w, b = matrix(kind, K, N, seed + i)
    out.append((w, b, 0, N))
  w, b = matrix(kind, 256, 200, seed + 50)
  out.append((w, b, 64, 72))
  return out


def h2_bytes(K, N):
  return -(-N // 128) * -(-K // 16) * 8192 + -(-N // 128) * 128 * 4


def host_pack(lib, w, b, col0, N):
  """{'plain', 'split', 'h2' (None: refused), 'bias'}: the host packers' bytes for the window."""
  from epos_amd import net_modes
  win = net_modes._fold(np.ascontiguousarray(w[:, col0:col0 + N]), np.ones(N, np.float32), 4)
  out = {'plain': net_modes._pack(lib.epos_pack_pointwise_weights, win, np.float32),
         'split': net_modes._pack(lib.epos_pack_pointwise_weights_split, win, np.uint8),
         'h2': net_modes._pack(lib.epos_pack_pointwise_weights_h2, win, np.uint8),
         'bias': net_modes._bias(b[col0:col0 + N], N, 128)}
  return {k: (v.view(np.uint8) if v is not None else None) for k, v in out.items()}


def device_pack(lib, probs, want=('plain', 'split', 'h2', 'bias')):
  """One grouped epos_pack_weights_device_f32 call; destinations pre-filled with FILL.
  Returns (status int32 [count], [{name: uint8 array} per problem])."""
  import torch
  from epos_amd import _lib
  dev = torch.device('cuda:0')
  keep, dsts = [], []
  arr = (_lib.WeightPackArgs * len(probs))()
  for i, (w, b, col0, N) in enumerate(probs):
    K, ldw = w.shape
    wt = torch.from_numpy(np.ascontiguousarray(w)).to(dev)
    bt = torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    npad = -(-N // 128) * 128
    sizes = {'plain': -(-K // 32) * 32 * npad * 4, 'split': -(-N // 128) * -(-K // 16) * 12288,
             'h2': h2_bytes(K, N), 'bias': npad * 4}
    d = {k: torch.full((sizes[k],), FILL, dtype=torch.uint8, device=dev) for k in want}
    keep += [wt, bt]
    dsts.append(d)
    p = lambda k: ctypes.c_void_p(d[k].data_ptr()) if k in d else None      # noqa: E731
    arr[i] = _lib.WeightPackArgs(W=wt.data_ptr(), ldw=ldw, col0=col0, bias=bt.data_ptr(),
                                 plain=p('plain'), split=p('split'), h2=p('h2'),
                                 bias_pad=p('bias'), K=K, N=N)
  status = torch.full((len(probs),), -1, dtype=torch.int32, device=dev)
  stream = torch.cuda.current_stream(dev)
  _lib.check(lib.epos_pack_weights_device_f32(arr, len(probs), status.data_ptr(),
                                              ctypes.c_void_p(stream.cuda_stream)),
             'epos_pack_weights_device_f32')
  torch.cuda.synchronize()
  return status.cpu().numpy(), [{k: v.cpu().numpy() for k, v in d.items()} for d in dsts]
