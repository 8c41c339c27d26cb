"""Guarded placement of a kernel's arrays (tests/test_gpu_linear_paths.py, tests/test_gpu_kernel_paths.py).

Every array of a call -- operand or output -- lives inside a larger backing buffer filled with one quiet-NaN bit pattern:
guards before and after it (at least GUARD_ROWS rows' worth of its leading dimension for a matrix, GUARD_FLOATS floats
for a vector), the pad columns of an `ld > width` array, the other slots of a ring and the output rectangle itself.  A
kernel that reads outside a rectangle reads NaN; one that writes outside it changes a float that `untouched_outside`
compares bit for bit; one that skips an output element leaves the pattern where `unwritten` finds it.

An array is anything with the fields name, rows, width, ld, off, role ("in" | "out") and ring (slots; 1: no ring)."""
from collections import namedtuple

import torch

NAN_BITS = 0x7FC0DEAD                    # a quiet NaN no arithmetic produces
GUARD_ROWS, GUARD_FLOATS = 64, 64
RING, RING_PICK = 3, 1                   # a ring has three slots, a call reads (or writes) the second
DEV = "cuda:0"

Array = namedtuple("Array", "name rows width ld off role ring")


def pad4(n):
    return (-n) % 4


def ring_stride(a):
    """Floats between two slots of a ring: whole float4s, so that the slot alone never costs the 16-byte paths."""
    return a.rows * a.ld + pad4(a.rows * a.ld)


class Placed:
    """`a` inside its NaN-filled backing buffer.  view: the rectangle (of the picked ring slot); first: the same
    rectangle of ring slot 0, the tensor a wrapper is handed together with a slot; ptr: its address; base: its offset
    in buf.  vector: guards of GUARD_FLOATS floats instead of GUARD_ROWS rows."""

    def __init__(self, a, values, vector=False, pick=RING_PICK, dev=DEV):
        guard = GUARD_FLOATS if vector else GUARD_ROWS * a.ld
        guard += pad4(guard)
        stride = ring_stride(a) if a.ring > 1 else 0
        span = a.ring * stride if a.ring > 1 else a.rows * a.ld
        self.buf = torch.empty(guard + a.off + span + guard + 4, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.buf.view(torch.int32).fill_(NAN_BITS)
        base = guard + a.off
        shape, strides, start = (a.rows, a.width), (a.ld, 1), base + (pick if a.ring > 1 else 0) * stride
        self.view = self.buf.as_strided(shape, strides, start)
        self.first = self.buf.as_strided(shape, strides, base)
        if values is not None:
            self.view.copy_(values.reshape(shape))
        self.inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=dev)
        self.inside.as_strided(shape, strides, start).fill_(True)
        self.ptr = self.buf.data_ptr() + 4 * base
        assert self.ptr % 16 == 4 * a.off
        self.base, self.stride, self.pick = base, stride, pick
        self.before = self.buf.view(torch.int32).clone()
        self.array = a

    def untouched_outside(self):
        after = self.buf.view(torch.int32)
        if self.array.role == "in":
            return torch.equal(after, self.before)
        return torch.equal(after[~self.inside], self.before[~self.inside])

    def unchanged(self):
        """Not one float of the buffer changed, the rectangle included."""
        return torch.equal(self.buf.view(torch.int32), self.before)

    def unwritten(self):
        """Elements of the rectangle that still hold the NaN pattern."""
        return int((self.buf.view(torch.int32)[self.inside] == NAN_BITS).sum().item())
