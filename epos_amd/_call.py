"""The boundary between torch tensors and the C ABI of libepos_hip.so, stated once: a kernel
reads and writes through raw pointers, so what a wrapper gets wrong here is no Python exception
but memory the kernel does not own.

  ptr            tensor -> c_void_p: the only such conversion in epos_amd/.
  stream_handle  the current stream of a device, as torch and as the C entries take it.
  launch         the device guard, the stream and record_stream for what the wrapper made.
  need_device    refuse a host tensor, or a machine without a device.
  flat, rows     an input as the kernel reads it: dense and flat, or rows a constant stride apart.
  dense          a tensor the caller must hand over dense already.
  out, workspace an output or a workspace given by the caller, or a new one.

The wrappers off the hot path go through launch. The entries that replay on a stream the
pipeline owns -- EposNet's launches and plan build (net.py, net_modes.py, multiscale.py),
EposPipeline.launch / collect, CorrExtractor.count / fill, CorrOrderer.run, MeshProjector.run --
take ptr and stream_handle alone: they make no device current and record nothing, and so rely
on one device per process (dist.py sets it).
"""
import ctypes

from epos_amd._lib import EposError


def ptr(t, offset_elems=0):
  """c_void_p of t's first element, or of the one offset_elems behind it; None (NULL) for None."""
  if t is None:
    return None
  if not offset_elems:              # the replayed path converts ~60 a step: no element_size()
    return ctypes.c_void_p(t.data_ptr())
  return ctypes.c_void_p(t.data_ptr() + offset_elems * t.element_size())


def stream_handle(device):
  """(the current torch stream of `device`, its hipStream_t as the C entries take it)."""
  import torch
  stream = torch.cuda.current_stream(device)
  return stream, ctypes.c_void_p(stream.cuda_stream)


class launch(object):
  """with launch(device) as q: makes `device` current around the C calls, which take q.handle
  (q.stream is the torch stream). q.keep(...) notes the dense copies and temporaries the wrapper
  made, None ignored: they outlive the call, so each is record_stream'ed on the way out, after
  a refusal too (it launched nothing, and recording is harmless)."""

  def __init__(self, device):
    import torch
    self.stream, self.handle = stream_handle(device)
    self._guard = torch.cuda.device(device)
    self._kept = []

  def keep(self, *tensors):
    self._kept += [t for t in tensors if t is not None]

  def __enter__(self):
    self._guard.__enter__()
    return self

  def __exit__(self, *exc):
    try:
      self._guard.__exit__(*exc)
    finally:
      for t in self._kept:
        t.record_stream(self.stream)
    return False


def need_device(t, message):
  """EposError(message) when t is not on a device, or, for None, when there is no device."""
  import torch
  if not (torch.cuda.is_available() if t is None else t.is_cuda):
    raise EposError(message)


def flat(t, device, dtype, numel, what, where):
  """t dense and flattened after its check: on `device` (else EposError naming `where`, 'the
  losses'), of `dtype` (TypeError) and, unless numel is None, of numel values (ValueError)."""
  if t.device != device:
    raise EposError('%s is on %s, %s on %s' % (what, t.device, where, device))
  if t.dtype != dtype:
    raise TypeError('%s must be %s, got %s' % (what, dtype, t.dtype))
  t = t.contiguous().reshape(-1)
  if numel is not None and t.numel() != numel:
    raise ValueError('%s holds %d values, expected %d' % (what, t.numel(), numel))
  return t


def rows(t, width):
  """(tensor, row stride) of t [..., width]: a view whose rows lie a constant stride apart is
  taken as it is (a slice of a wider buffer), anything else is made dense."""
  if t.stride(-1) == 1:
    try:
      v = t.view(-1, width)
      if v.shape[0] < 2 or v.stride(0) >= width:
        return v, (v.stride(0) if v.shape[0] > 1 else width)
    except RuntimeError:
      pass
  return t.contiguous().view(-1, width), width


def dense(t, device, dtype, what, numel=None, shape=None, name=None):
  """ValueError unless t is a contiguous `dtype` tensor on `device` of numel values or of
  `shape`; name: how the message spells the dtype where not as torch does."""
  if (t.device != device or t.dtype != dtype or not t.is_contiguous() or
      (t.numel() != numel if shape is None else tuple(t.shape) != tuple(shape))):
    raise ValueError('%s must be a contiguous %s tensor of %s on %s' % (
        what, name or dtype,
        '%d values' % numel if shape is None else 'shape %s' % (tuple(shape),), device))


def out(t, device, dtype, shape, what, flat=False, rows=False):
  """The output tensor t after its check, or a new one for None: a contiguous `dtype` tensor of
  `shape` on `device` -- flat: of as many values in any shape; rows: [..., shape[-1]], which the
  caller passes through rows() -- else ValueError."""
  import torch
  if t is None:
    return torch.empty(shape, dtype=dtype, device=device)
  if rows:
    fits = t.shape[-1] == shape[-1]
  elif flat:
    fits = t.is_contiguous() and t.numel() == torch.Size(shape).numel()
  else:
    fits = t.is_contiguous() and tuple(t.shape) == tuple(shape)
  if t.device != device or t.dtype != dtype or not fits:
    raise ValueError('%s must be a %s%s tensor of shape %s on %s' % (
        what, '' if rows else 'contiguous ', dtype,
        '[..., %d]' % shape[-1] if rows else tuple(shape), device))
  return t


def workspace(t, device, nbytes, dtype=None):
  """The workspace tensor t after its check, or a new one for None: contiguous, on `device`, of
  at least nbytes bytes and, where one is given, of `dtype` (a new one: int64), else
  ValueError."""
  import torch
  if t is None:
    new = dtype or torch.int64
    return torch.empty((max(-(-nbytes // new.itemsize), 1),), dtype=new, device=device)
  if (t.device != device or not t.is_contiguous() or (dtype is not None and t.dtype != dtype) or
      t.numel() * t.element_size() < nbytes):
    raise ValueError('workspace must be a contiguous %stensor of at least %d bytes on %s' % (
        '%s ' % dtype if dtype else '', nbytes, device))
  return t
