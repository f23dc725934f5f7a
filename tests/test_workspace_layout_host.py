"""CPU: mdm_workspace_layout / mdm_workspace_field_name describe the workspace that carve() (csrc/model.hip) lays out, from the
one table that carves it.  No GPU: the model struct is filled by hand (only D, F, L, H, E, Dt enter the layout; `layers` must be
non-NULL for the model check and is never dereferenced)."""
import ctypes as C

import pytest

from conftest import pkg

WIDTHS = {"small": dict(D=512, F=1024, Dt=256, H=4, E=8, L=1), "big": dict(D=1024, F=2048, Dt=512, H=4, E=16, L=2)}
SHAPES = [(1, 2, 1), (3, 50, 5), (2, 196, 85)]
INT_FIELDS = {"top_idx", "perm", "pos4", "hist", "goff", "cursor", "len_low"}


def _lib():
    L = pkg("_lib")
    import os
    if not os.path.exists(L.LIB_PATH):
        pkg("build").build(verbose=False)
    return L, L.lib()


def _model(L, dims):
    m = L.Model()
    for k, v in dims.items():
        setattr(m, k, v)
    m.feats, m.num_frames = 263, 196
    layers = (L.Layer * (2 * dims["L"]))()
    m.layers = C.cast(layers, C.POINTER(L.Layer))
    return m, layers


def _layout(lib, m, B, T, N, cap=None):
    n = lib.mdm_workspace_layout(C.byref(m), B, T, N, None, None, None, 0)
    assert n > 0
    cap = n if cap is None else cap
    off, size, kind = (C.c_int64 * n)(*[-7] * n), (C.c_int64 * n)(*[-7] * n), (C.c_int32 * n)(*[-7] * n)
    assert lib.mdm_workspace_layout(C.byref(m), B, T, N, off, size, kind, cap) == n
    return n, list(off), list(size), list(kind)


def _names(lib, n):
    return [lib.mdm_workspace_field_name(i).decode() for i in range(n)]


@pytest.mark.parametrize("B,T,N", SHAPES)
@pytest.mark.parametrize("width", sorted(WIDTHS))
def test_fields_are_aligned_ordered_disjoint_and_end_at_workspace_bytes(width, B, T, N):
    L, lib = _lib()
    m, keep = _model(L, WIDTHS[width])
    n, off, size, kind = _layout(lib, m, B, T, N)
    need = lib.mdm_workspace_bytes(C.byref(m), B, T, N)
    assert need > 0 and n >= 40
    assert off[0] == 0
    end = 0
    for i in range(n):
        assert off[i] % 256 == 0 and size[i] > 0, (i, off[i], size[i])
        assert off[i] >= end, (i, off[i], end)        # increasing, no overlap
        assert off[i] - end < 256, (i, off[i], end)   # and nothing but the alignment gap between neighbours
        end = off[i] + size[i]
    assert (end + 255) // 256 * 256 == need
    names = _names(lib, n)
    assert {nm for nm, k in zip(names, kind) if k == 1} == INT_FIELDS
    assert set(kind) == {0, 1}
    # the sizes the header documents for the router's buffers (M = B * T rows, 2 E expert groups)
    by = dict(zip(names, size))
    M, E, D = B * T, WIDTHS[width]["E"], WIDTHS[width]["D"]
    assert by["top_idx"] == by["perm"] == by["pos4"] == 4 * M * 4
    assert by["goff"] == (2 * E + 1) * 4 and by["cursor"] == 2 * E * 4 and by["len_low"] == B * 4
    assert by["xa"] == M * D * 4 and by["xa16"] == M * D * 2 and by["hn"] == 2 * M * D * 4


def test_the_existing_aids_point_at_the_same_fields():
    """mdm_route_workspace / mdm_expert_workspace report offsets of fields by name: the layout agrees with them."""
    L, lib = _lib()
    m, keep = _model(L, WIDTHS["small"])
    B, T, N = 3, 50, 5
    n, off, _, _ = _layout(lib, m, B, T, N)
    by = dict(zip(_names(lib, n), off))
    r, e = (C.c_int64 * 8)(), (C.c_int64 * 3)()
    assert lib.mdm_route_workspace(C.byref(m), B, T, N, r) == 0 and lib.mdm_expert_workspace(C.byref(m), B, T, N, e) == 0
    assert list(r) == [by[k] for k in ("hn", "top_idx", "top_val", "perm", "rowscale", "pos4", "goff", "cursor")]
    assert list(e) == [by[k] for k in ("hn_scale", "hid", "y2")]


def test_cap_limits_what_is_written():
    L, lib = _lib()
    m, keep = _model(L, WIDTHS["small"])
    full = _layout(lib, m, 3, 50, 5)
    n, off, size, kind = _layout(lib, m, 3, 50, 5, cap=5)
    assert n == full[0]
    assert off[:5] == full[1][:5] and size[:5] == full[2][:5] and kind[:5] == full[3][:5]
    assert off[5:] == [-7] * (n - 5) and size[5:] == [-7] * (n - 5) and kind[5:] == [-7] * (n - 5)


def test_bad_arguments_return_minus_one():
    L, lib = _lib()
    m, keep = _model(L, WIDTHS["small"])
    buf = (C.c_int64 * 64)()
    k = (C.c_int32 * 64)()
    assert lib.mdm_workspace_layout(None, 1, 2, 1, buf, buf, k, 64) == -1
    assert lib.mdm_workspace_layout(C.byref(m), 0, 2, 1, buf, buf, k, 64) == -1
    assert lib.mdm_workspace_layout(C.byref(m), 1, 0, 1, buf, buf, k, 64) == -1
    assert lib.mdm_workspace_layout(C.byref(m), 1, 2, 1, None, buf, k, 64) == -1


def test_the_fills_and_guards_of_scratch_hygiene():
    """tests/scratch_hygiene.py on CPU tensors with a real layout: P is 0xFF (NaN in every float format) in every data field and in
    the gaps, the donor's bytes in every int field; D is the donor; a byte written on either side of a window breaks its guards."""
    import torch
    import scratch_hygiene as SH
    L, lib = _lib()
    m, keep = _model(L, WIDTHS["small"])
    B, T, N = 1, 2, 1
    layout = SH.workspace_layout(m, B, T, N)
    need = lib.mdm_workspace_bytes(C.byref(m), B, T, N)
    g = SH.guarded(need, guard=1024, device="cpu")
    assert g.win.numel() == need and g.buf.numel() == need + 2048 and g.guards_untouched()
    donor = (torch.arange(need, dtype=torch.int64) % 251).to(torch.uint8)  # never 0xFF
    SH.fill_window(g.win, "P", layout, donor)
    covered = torch.zeros(need, dtype=torch.bool)
    for name, off, size, kind in layout:
        field = g.win[off:off + size]
        covered[off:off + size] = True
        if kind == 1:
            assert torch.equal(field, donor[off:off + size]), name
        else:
            assert bool((field == 0xFF).all()), name
            assert bool(torch.isnan(field.view(torch.float32)).all()) and bool(torch.isnan(field.view(torch.bfloat16)).all()), name
            assert bool(torch.isnan(field.view(torch.float16)).all()) and bool(torch.isnan(field.view(torch.float8_e4m3fn).float()).all())
    assert bool((g.win[~covered] == 0xFF).all()) and int((~covered).sum()) > 0  # the alignment gaps
    assert SH.poison_fraction(g.win, layout)["xa"] == 1.0 and SH.poison_fraction(g.win, layout)["perm"] == 0.0
    SH.fill_window(g.win, "D", layout, donor)
    assert torch.equal(g.win, donor)
    SH.fill_window(g.win, "Z")
    assert not g.win.any() and g.guards_untouched()
    for at in (1023, 1024 + need):  # the byte in front of the window, the byte behind it
        g.buf[at] ^= 1
        assert not g.guards_untouched()
        g.buf[at] ^= 1
    g.buf[1024] ^= 1  # inside the window: not a guard
    assert g.guards_untouched()
    gl, t = SH.guarded_like((3, 5), fill=7.0, guard=512, device="cpu")
    assert t.shape == (3, 5) and bool((t == 7.0).all()) and gl.guards_untouched() and gl.nbytes == 60


def test_names_are_non_empty_and_unique():
    L, lib = _lib()
    m, keep = _model(L, WIDTHS["big"])
    n = lib.mdm_workspace_layout(C.byref(m), 1, 2, 1, None, None, None, 0)
    names = _names(lib, n)
    assert all(names) and len(set(names)) == n
    assert INT_FIELDS <= set(names)
    assert lib.mdm_workspace_field_name(n) == b"" and lib.mdm_workspace_field_name(-1) == b""
