"""Scratch buffers under test (tests/test_workspace_hygiene_gpu.py, tests/test_scratch_hygiene_gpu.py).

Every scratch-taking C entry works out of a caller's buffer that is never cleared.  `guarded` hands an entry a window of exactly the
size its query returns between two sentinel-filled guards: a write past either end breaks a guard (`guards_untouched`, compared bit
for bit).  The fills put different histories into the window before a call; a result that differs between two fills comes from a
read of scratch the call did not write itself:

  Z  zeros;
  D  the bytes a donor run left there (another input, another precision mode: finite values of another format);
  P  poison: 0xFF bytes -- NaN as fp32, bf16, fp16 and e4m3 -- in every data field and in the alignment gaps between fields, the
     donor's bytes in the int fields.  Poison never goes into an int field, so that no stale value can be turned into an address;
     whether a stale index is read is judged by Z against D, whose indices are in range for the shape."""
from __future__ import annotations

import ctypes as C

import torch

GUARD_BYTE = 0x5A
POISON_BYTE = 0xFF
ERR_ARG = 1  # MDM_ERR_ARG


class Guarded:
    """A uint8 allocation guard | window | guard; `win` is the window (nbytes, at a 512-byte aligned address)."""

    def __init__(self, nbytes, guard=1 << 20, device="cuda"):
        assert guard % 512 == 0 and nbytes >= 0
        self.nbytes, self.guard = int(nbytes), guard
        self.buf = torch.full((guard + self.nbytes + guard,), GUARD_BYTE, dtype=torch.uint8, device=device)
        self.win = self.buf[guard:guard + self.nbytes]
        assert self.win.data_ptr() % 512 == 0 or device == "cpu"

    def guards_untouched(self) -> bool:
        g = self.guard
        return bool((self.buf[:g] == GUARD_BYTE).all()) and bool((self.buf[g + self.nbytes:] == GUARD_BYTE).all())

    def typed(self, dtype, shape):
        """The window as a tensor of `dtype` and `shape` (which must fill it exactly)."""
        return self.win.view(dtype).view(shape)

    def ptr(self):
        return self.win.data_ptr()


def guarded(nbytes, guard=1 << 20, device="cuda") -> Guarded:
    return Guarded(nbytes, guard, device)


def guarded_like(shape, dtype=torch.float32, fill=None, guard=1 << 20, device="cuda"):
    """(Guarded, tensor view of its window) for an output of `shape`; `fill` = sentinel value put into the window."""
    n = 1
    for s in shape:
        n *= int(s)
    g = Guarded(n * torch.empty((), dtype=dtype).element_size(), guard, device)
    t = g.typed(dtype, tuple(shape))
    if fill is not None:
        t.fill_(fill)
    return g, t


def workspace_layout(model_struct, B, T, N):
    """[(name, byte offset, byte size, kind)] of the workspace carved for (model, B, T, N), from mdm_workspace_layout."""
    from conftest import pkg
    lib = pkg("_lib").lib()
    n = lib.mdm_workspace_layout(C.byref(model_struct), B, T, N, None, None, None, 0)
    assert n > 0
    off, size, kind = (C.c_int64 * n)(), (C.c_int64 * n)(), (C.c_int32 * n)()
    assert lib.mdm_workspace_layout(C.byref(model_struct), B, T, N, off, size, kind, n) == n
    return [(lib.mdm_workspace_field_name(i).decode(), off[i], size[i], kind[i]) for i in range(n)]


def copy_int_fields(win: torch.Tensor, layout, donor: torch.Tensor):
    """The int fields of `layout` in the window take the donor's bytes; everything else stays."""
    for _, off, size, kind in layout:
        if kind == 1:
            win[off:off + size].copy_(donor[off:off + size])


def fill_window(win: torch.Tensor, how: str, layout=None, donor: torch.Tensor = None):
    """Put fill Z, D or P (see the module docstring) into a workspace window; a window longer than the layout (and than the donor)
    keeps zeros (Z, D) or poison (P) behind it."""
    if how == "Z":
        win.zero_()
    elif how == "D":
        win.zero_()
        win[:donor.numel()].copy_(donor)
    elif how == "P":
        win.fill_(POISON_BYTE)
        copy_int_fields(win, layout, donor)
    else:
        raise ValueError(how)


def fill_float_scratch(win: torch.Tensor, how: str):
    """The two fills of a float-only scratch: zeros, 0xFF bytes."""
    win.fill_(0 if how == "Z" else POISON_BYTE)


def poison_fraction(win: torch.Tensor, layout):
    """{field: fraction of its bytes that still hold the poison byte} -- where a call left a field unwritten (diagnostics)."""
    return {name: float((win[off:off + size] == POISON_BYTE).float().mean()) for name, off, size, _ in layout}
