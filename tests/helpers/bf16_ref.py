"""numpy restatement of fp32 -> bf16 rounding (round to nearest, ties to even) for the bf16-mode
tests: the bit patterns the packer and the kernels must produce, and the rounded values."""
import numpy as np


def bf16_round_bits(x):
  """uint16 bf16 bit patterns of fp32 `x` (RNE; NaN stays a quiet NaN)."""
  u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
  nan = (u & 0x7fffffff) > 0x7f800000
  r = (u + 0x7fff + ((u >> 16) & 1)) >> 16
  r = np.where(nan, (u >> 16) | 0x40, r)
  return r.astype(np.uint16)


def bf16_to_f32(bits):
  return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
  """fp32 values of RNE-rounded `x`."""
  return bf16_to_f32(bf16_round_bits(x))
