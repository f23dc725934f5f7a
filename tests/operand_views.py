"""Operand windows for the GEMM / fused-MLP tests (CPU-only code; tests/test_operand_views_gpu.py runs it on the device and
tests/test_operand_views_host.py proves on the CPU that its assertions can see a wrong stride).

MdmGemmDesc / MdmMlpDesc describe every operand by a pointer and a leading dimension.  A `Win` is such an operand inside a
larger allocation: `buffer` is [rows + pad_rows, ld] filled with a poison (inputs: NaN, fp8 bytes 0x7f = NaN in e4m3) or a
sentinel (outputs: 7.0, fp8 bytes 0x55), `view = buffer[:rows, col0:col0 + cols]` is what the kernel is given.  A read outside
the window turns the result NaN, a write outside it breaks the sentinel (`outside_untouched`, compared bit for bit).

  aligned windows: col0 = 32, ld = cols + a multiple of 32, different for R1 / R2 / C (N + 64 / N + 96 / N + 32): every base
                   pointer stays 16-byte aligned, so a kernel keeps the path it takes on the dense copy and the two runs
                   must agree in every bit;
  odd windows:     col0 = 0 and ld = cols + 1 (or + 3): the base stays aligned, only the leading dimension is odd.

`GemmCase` / `build_gemm` describe and build the operands of one C = epilogue(A W^T) launch, `emulate_gemm` is a torch
emulation of that launch through explicit (pointer offset, ld) pairs with one switch per stride bug (MUTANTS), and `check_case`
holds the assertions both test files apply."""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from types import SimpleNamespace

import torch

NAN = float("nan")
FP8_NAN = 0x7F
SENTINEL = {torch.float32: 7.0, torch.bfloat16: 7.0, torch.float16: 7.0, torch.uint8: 0x55}
PAD_ROWS = 3
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.uint8: torch.uint8}
H16 = {"bf16": torch.bfloat16, "f16": torch.float16}


def bits(t: torch.Tensor) -> torch.Tensor:
    """The integer view of a tensor: NaN == NaN and -0 != +0 there."""
    return t.view(_INT[t.dtype])


def window(rows, cols, *, ld, col0=0, pad_rows=PAD_ROWS, dtype=torch.float32, fill=NAN, device="cpu"):
    """(buffer [rows + pad_rows, ld] filled with `fill`, view = buffer[:rows, col0:col0 + cols])."""
    assert ld >= col0 + cols and rows >= 0 and pad_rows >= 0
    buffer = torch.full((rows + pad_rows, ld), fill, dtype=dtype, device=device)
    return buffer, buffer[:rows, col0:col0 + cols]


def outside_untouched(buffer: torch.Tensor, view_spec, sentinel=None) -> bool:
    """Every element of `buffer` outside the window view_spec = (rows, cols, col0) still holds the sentinel, bit for bit."""
    rows, cols, col0 = view_spec
    s = SENTINEL[buffer.dtype] if sentinel is None else sentinel
    want = bits(torch.full((1,), s, dtype=buffer.dtype, device=buffer.device))
    outside = torch.ones(buffer.shape, dtype=torch.bool, device=buffer.device)
    outside[:rows, col0:col0 + cols] = False
    return bool((bits(buffer)[outside] == want).all())


class Win:
    """One operand window (see the module docstring)."""

    def __init__(self, rows, cols, *, ld, col0=0, pad_rows=PAD_ROWS, dtype=torch.float32, fill=NAN, device="cpu"):
        self.rows, self.cols, self.ld, self.col0, self.pad_rows, self.fill = rows, cols, ld, col0, pad_rows, fill
        self.buffer, self.view = window(rows, cols, ld=ld, col0=col0, pad_rows=pad_rows, dtype=dtype, fill=fill, device=device)

    @property
    def spec(self):
        return self.rows, self.cols, self.col0

    @property
    def dtype(self):
        return self.buffer.dtype

    def put(self, values):
        self.view.copy_(values)
        return self

    def _like(self, ld, col0, device):
        return Win(self.rows, self.cols, ld=ld, col0=col0, pad_rows=self.pad_rows, dtype=self.dtype, fill=self.fill, device=device)

    def to(self, device):
        """A copy of the whole allocation (poison included) on `device`."""
        w = self._like(self.ld, self.col0, device)
        w.buffer.copy_(self.buffer)
        return w

    def dense(self, device=None):
        """The same values as a contiguous operand (ld = cols, col0 = 0); the pad rows behind it keep the fill."""
        return self._like(self.cols, 0, device or self.buffer.device).put(self.view)

    def untouched(self) -> bool:
        return outside_untouched(self.buffer, self.spec, self.fill)


def in_aligned(rows, cols, dtype=torch.float32, extra=64, fill=NAN):
    return Win(rows, cols, ld=cols + extra, col0=32, dtype=dtype, fill=fill)


def out_window(rows, cols, dtype, ld, col0):
    return Win(rows, cols, ld=ld, col0=col0, dtype=dtype, fill=SENTINEL[dtype])


def offset_vector(values: torch.Tensor, lead: int = 1) -> torch.Tensor:
    """`values` as a slice starting `lead` elements into a longer NaN vector (a bias / colscale that is not 16-byte aligned)."""
    long = torch.full((values.numel() + lead + 7,), NAN, dtype=values.dtype, device=values.device)
    long[lead:lead + values.numel()] = values.reshape(-1)
    return long[lead:lead + values.numel()]


def x2_rows(x: torch.Tensor) -> torch.Tensor:
    """fp32 [M, K] -> MDM_OP_X2_ROW rows [M, 2 K] bf16: per 32 columns, 32 hi then 32 lo = rn(x - hi)."""
    M, K = x.shape
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return torch.stack([hi.reshape(M, K // 32, 32), lo.reshape(M, K // 32, 32)], 2).reshape(M, 2 * K).contiguous()


def x2_value(rows16: torch.Tensor) -> torch.Tensor:
    """MDM_OP_X2_ROW rows [M, 2 K] -> hi + lo in fp64 [M, K]."""
    M = rows16.shape[0]
    p = rows16.double().reshape(M, -1, 2, 32)
    return (p[:, :, 0] + p[:, :, 1]).reshape(M, -1)


def rel_inf(a, b) -> float:
    """||a - b||_inf / ||b||_inf (the metric of tests/conftest.py); NaN anywhere gives NaN, which passes no gate."""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


ACTS = {"none": lambda v: v, "gelu": torch.nn.functional.gelu, "silu": torch.nn.functional.silu,
        "feat": lambda v: 0.1 * torch.exp(v.clamp(-15, 15))}


# ---- the assertions both test files apply ----------------------------------------------------------------------------------------
Out = SimpleNamespace  # name, got (window of the view run), dense (the dense run's result or None), ref (fp64 or None), tol


class ViewCheckError(AssertionError):
    def __init__(self, which, message):
        super().__init__(f"[{which}] {message}")
        self.which = which


def check_case(label, outs, canaries, derived=()):
    """The checks of one view run, in this order:
      canary     every output buffer is bit-unchanged outside its window;
      finite     no output holds a NaN / Inf (a read of the NaN poison around an input window);
      bit-equal  the window equals the dense run of the same kernel (outs[i].dense, where given);
      derived    pairs (name, got, want) that must agree in every bit (the 16-bit copy is the rounded fp32 result, Cx2 its split);
      gate       rel_inf against fp64 of the identically rounded operands within the dense test's tolerance.
    Raises ViewCheckError naming the first that fails; returns {output name: measured error} and prints one line."""
    for w in canaries:
        if not w.untouched():
            raise ViewCheckError("canary", f"{label}: a write outside the window {w.spec} of a [{tuple(w.buffer.shape)}] buffer")
    def as_float(x):
        return x.view(torch.float8_e4m3fn).float() if x.dtype == torch.uint8 else x.float() if x.dtype != torch.float64 else x

    for o in outs:
        v = as_float(o.got)
        if not bool(torch.isfinite(v).all()):
            raise ViewCheckError("finite", f"{label}: {o.name} holds {int((~torch.isfinite(v)).sum())} non-finite values")
    equal = None
    for o in outs:
        if o.dense is not None:
            equal = True
            if not torch.equal(bits(o.got), bits(o.dense)):
                raise ViewCheckError("bit-equal", f"{label}: {o.name} differs from the dense run in "
                                                  f"{int((bits(o.got) != bits(o.dense)).sum())} elements")
    for name, got, want in derived:
        if not torch.equal(bits(got), bits(want)):
            raise ViewCheckError("derived", f"{label}: {name} differs in {int((bits(got) != bits(want)).sum())} elements")
    errs = {}
    for o in outs:
        if o.ref is not None:
            errs[o.name] = rel_inf(as_float(o.got).cpu(), o.ref.cpu())
            if not errs[o.name] < o.tol:
                raise ViewCheckError("gate", f"{label}: {o.name} is {errs[o.name]:.3e} from fp64, gate {o.tol:.1e}")
    print(f"{label}: view == dense {'yes' if equal else 'n/a'}; vs fp64 " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    return errs


# ---- one C = epilogue(A W^T) launch ----------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GemmCase:
    name: str
    M: int
    N: int
    K: int
    a_fmt: str                # "bf16" | "f16" (16-bit rows), "f32" (fp32 rows), "x2" (MDM_OP_X2_ROW rows)
    precision: int            # MdmGemmDesc.precision
    layout: str = "aligned"   # | "odd_ldc" (N + 1) | "odd_ldr1" (N + 3) | "ragged" (ldc = N rounded up to 16) | "vec_off" (bias / colscale + 4 B)
    sizes: tuple = ()         # grouped mode: rows per group (sum = M)
    gather: bool = False      # rows gathered from a source of `src_rows` rows
    src_rows: int = 0
    act: str = "none"
    colscale: bool = False
    rowscale: bool = False
    alpha: float = 1.0
    out_scale: float = 1.0
    r1: bool = False
    r1_scale: float = 1.0
    r1_mod: int = 0
    r2: bool = False
    out32: bool = True
    out16: bool = False
    outx2: bool = False
    tol32: float = 1e-4
    tol16: float = 1e-2

    @property
    def ldc(self):
        return {"aligned": self.N + 32, "vec_off": self.N + 32, "odd_ldr1": self.N + 32, "odd_ldc": self.N + 1,
                "ragged": (self.N + 15) // 16 * 16}[self.layout]


def _uniform(g, *shape, scale=1.0):
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def build_gemm(c: GemmCase):
    """The operands of a case on the CPU: input windows in NaN-poisoned buffers, output windows in sentinel-filled ones, the fp32
    weight / bias the test packs, and the fp64 reference of the identically rounded operands."""
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    G = max(len(c.sizes), 1)
    assert not c.sizes or sum(c.sizes) == c.M
    S = c.src_rows if c.gather else c.M
    x = _uniform(g, S, c.K)
    w = _uniform(g, G, c.N, c.K, scale=c.K ** -0.5 * 2)
    b = _uniform(g, G, c.N)
    t = SimpleNamespace(case=c, w=w, b=b, G=G)
    aligned_c = c.layout in ("aligned", "vec_off", "odd_ldr1")
    # A: rows of the format the kernel reads; `xv` = the values it sees, in fp64
    if c.a_fmt in H16:
        x16 = x.to(H16[c.a_fmt])
        t.A, t.xv = in_aligned(S, c.K, H16[c.a_fmt]).put(x16), x16.double()
    elif c.a_fmt == "f32":
        t.A, t.xv = in_aligned(S, c.K).put(x), x.double()
    else:  # pre-split rows: 2 K 16-bit elements per row, ld and col0 twice those of the fp32 rows they replace
        rows = x2_rows(x)
        t.A = Win(S, 2 * c.K, ld=2 * (c.K + 64), col0=64, dtype=torch.bfloat16).put(rows)
        t.xv = x2_value(rows)
    t.wv = (w.to(H16[c.a_fmt]) if c.a_fmt in H16 else w).double()
    t.gather = torch.randint(0, S, (c.M,), generator=g, dtype=torch.int32) if c.gather else None
    sizes = c.sizes or (c.M,)
    t.goff = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0)), dtype=torch.int32)
    t.bias = offset_vector(b.reshape(-1)) if c.layout == "vec_off" else b.reshape(-1).clone()
    cs = _uniform(g, c.N)
    t.colscale = (offset_vector(cs) if c.layout == "vec_off" else cs) if c.colscale else None
    t.rowscale = _uniform(g, c.M).abs() + 0.1 if c.rowscale else None
    t.R1 = t.R2 = t.C = t.C16 = t.Cx2 = None
    # the ragged layout keeps ldr1 / ldr2 multiples of 4 (as its ldc), so that only the N edge takes the kernels off their vector path
    ragged = (c.N + 15) // 16 * 16 - c.N if c.layout == "ragged" else 0
    if c.r1:
        r1_rows = c.r1_mod or c.M
        t.R1 = (Win(r1_rows, c.N, ld=c.N + 3, col0=0) if c.layout == "odd_ldr1" else in_aligned(r1_rows, c.N, extra=64 + ragged))
        t.R1.put(_uniform(g, r1_rows, c.N))
    if c.r2:
        t.R2 = in_aligned(c.M, c.N, extra=96 + ragged).put(_uniform(g, c.M, c.N))
    col0 = 32 if aligned_c else 0
    if c.out32:
        t.C = out_window(c.M, c.N, torch.float32, c.ldc, col0)
    if c.out16:
        t.C16 = out_window(c.M, c.N, H16.get(c.a_fmt, torch.bfloat16), c.ldc, col0)
    if c.outx2:  # starts 2 col0 16-bit elements in, row stride 2 ldc
        t.Cx2 = out_window(c.M, 2 * c.N, torch.bfloat16, 2 * c.ldc, 2 * col0)
    # fp64 reference
    xs = t.xv[t.gather.long()] if c.gather else t.xv
    ref = torch.empty(c.M, c.N, dtype=torch.float64)
    for e in range(G):
        r = slice(int(t.goff[e]), int(t.goff[e + 1]))
        ref[r] = xs[r] @ t.wv[e].T + b[e].double()
    ref = ACTS[c.act](c.alpha * ref) * c.out_scale
    if c.colscale:
        ref = ref * t.colscale.double()[None]
    if c.rowscale:
        ref = ref * t.rowscale.double()[:, None]
    if c.r1:
        ref = ref + c.r1_scale * t.R1.view.double()[torch.arange(c.M) % r1_rows]
    if c.r2:
        ref = ref + t.R2.view.double()
    t.ref = ref
    return t


_WINS = ("A", "R1", "R2", "C", "C16", "Cx2")
_VECS = ("bias", "colscale", "rowscale", "gather", "goff")


def on_device(t, device, dense=False):
    """The operands of build_gemm on `device`: as they are (whole allocations, poison included), or as contiguous copies of the
    same values with fresh sentinel-filled outputs (dense)."""
    d = SimpleNamespace(**vars(t))
    for k in _WINS:
        w = getattr(t, k)
        if w is not None:
            setattr(d, k, w.dense(device) if dense else w.to(device))
    for k in _VECS:
        v = getattr(t, k)
        if v is None:
            continue
        if dense or v.storage_offset() == 0:
            setattr(d, k, v.contiguous().clone().to(device))
        else:  # a slice into a longer vector: move the whole vector, slice again
            base = torch.empty(0, dtype=v.dtype).set_(v.untyped_storage()).to(device)
            setattr(d, k, base[v.storage_offset():v.storage_offset() + v.numel()])
    return d


def gemm_checks(label, view, dense=None):
    """check_case for one launch of a GemmCase: `view` / `dense` are the operand sets (on_device) after the two runs."""
    c = view.case
    outs, derived = [], []
    for k, tol in (("C", c.tol32), ("C16", c.tol16)):
        w = getattr(view, k)
        if w is not None:
            outs.append(Out(name=k, got=w.view, dense=getattr(dense, k).view if dense is not None else None, ref=view.ref, tol=tol))
    if view.Cx2 is not None:
        outs.append(Out(name="Cx2", got=view.Cx2.view, dense=dense.Cx2.view if dense is not None else None, ref=None, tol=None))
        if view.C is not None:
            derived.append(("Cx2 vs split(C)", view.Cx2.view, x2_rows(view.C.view.contiguous())))
        else:
            outs.append(Out(name="Cx2 value", got=x2_value(view.Cx2.view).float(), dense=None, ref=view.ref, tol=c.tol32))
    if view.C is not None and view.C16 is not None:
        derived.append(("C16 vs round(C)", view.C16.view, view.C.view.to(view.C16.dtype)))
    return check_case(label, outs, [w for w in (view.C, view.C16, view.Cx2) if w is not None], derived)


# ---- the emulation and its switches ----------------------------------------------------------------------------------------------
MUTANTS = {
    "a_stride_k": "A read with row stride K instead of A.ld",
    "c_stride_n": "C written with row stride N instead of ldc",
    "r1_uses_ldc": "R1 read with ldc instead of ldr1",
    "r2_uses_ldr1": "R2 read with ldr1 instead of ldr2",
    "r1_mod_ignored": "R1 row m instead of m mod r1_mod",
    "c16_dense_stride": "the 16-bit copy written with its own dense row stride",
    "cx2_stride_ldc": "Cx2 written with row stride ldc instead of 2 ldc",
    "quad_spill": "a whole quad stored at the ragged N edge",
    "gather_dense_row": "a gathered row taken from the dense row index",
}


def _read(win: Win, ld, rows):
    """`rows` x win.cols elements at (pointer offset win.col0, row stride ld) of the flat allocation; an access behind the
    allocation reads poison (it stands for whatever lies there)."""
    flat = win.buffer.reshape(-1)
    need = win.col0 + (rows - 1) * ld + win.cols
    if need > flat.numel():
        flat = torch.cat([flat, torch.full((need - flat.numel(),), win.fill, dtype=flat.dtype)])
    return flat.as_strided((rows, win.cols), (ld, 1), win.col0)


def _write(win: Win, ld, values):
    flat = win.buffer.reshape(-1)
    rows, cols = values.shape
    assert win.col0 + (rows - 1) * ld + cols <= flat.numel(), "the emulation never writes behind an allocation"
    flat.as_strided((rows, cols), (ld, 1), win.col0).copy_(values)


def emulate_gemm(t, mutant=None):
    """C = epilogue(A W^T) of build_gemm's operands in fp64, read and written through (pointer offset, ld) pairs; `mutant` names
    one switch of MUTANTS.  Writes t.C / t.C16 / t.Cx2 in place."""
    assert mutant is None or mutant in MUTANTS
    c = t.case
    rows = torch.arange(c.M)
    src = t.gather.long() if (c.gather and mutant != "gather_dense_row") else rows
    a = _read(t.A, t.A.cols if mutant == "a_stride_k" else t.A.ld, max(t.A.rows, int(src.max()) + 1))[src]
    a = x2_value(a) if c.a_fmt == "x2" else a.double()
    v = torch.empty(c.M, c.N, dtype=torch.float64)
    for e in range(t.G):
        r = slice(int(t.goff[e]), int(t.goff[e + 1]))
        v[r] = a[r] @ t.wv[e].T + t.bias.double()[e * c.N:(e + 1) * c.N]
    v = ACTS[c.act](c.alpha * v) * c.out_scale
    if t.colscale is not None:
        v = v * t.colscale.double()[None]
    if t.rowscale is not None:
        v = v * t.rowscale.double()[:, None]
    ldc = t.C.ld if t.C is not None else t.C16.ld if t.C16 is not None else t.Cx2.ld // 2  # (the dense copies have their own)
    if t.R1 is not None:
        mr = rows % c.r1_mod if (c.r1_mod and mutant != "r1_mod_ignored") else rows
        v = v + c.r1_scale * _read(t.R1, ldc if mutant == "r1_uses_ldc" else t.R1.ld, int(mr.max()) + 1)[mr].double()
    if t.R2 is not None:
        v = v + _read(t.R2, t.R1.ld if mutant == "r2_uses_ldr1" else t.R2.ld, c.M).double()
    v = v.float()
    if mutant == "quad_spill" and c.N % 4:  # the last lane stores its four columns; those past N hold the clamped column's value
        v = torch.cat([v, v[:, -1:].expand(-1, 4 - c.N % 4)], 1)
    if t.C is not None:
        _write(t.C, c.N if mutant == "c_stride_n" else ldc, v)
    if t.C16 is not None:
        _write(t.C16, c.N if mutant == "c16_dense_stride" else ldc, v.to(t.C16.dtype))
    if t.Cx2 is not None:
        _write(t.Cx2, ldc if mutant == "cx2_stride_ldc" else 2 * ldc, x2_rows(v))


# ---- the cases of the GEMM kernels (tests/test_operand_views_gpu.py runs them, the host test mutates them) ------------------------
_FULL = dict(act="gelu", colscale=True, rowscale=True, alpha=0.9, out_scale=0.5, r1=True, r1_scale=0.3, r2=True, out16=True)
_EPI = dict(colscale=True, rowscale=True, alpha=0.7, out_scale=0.3, r1=True, r1_scale=0.25, r1_mod=50, r2=True)
_STREAM = dict(act="gelu", colscale=True, alpha=0.9, out_scale=0.5, r1=True, r1_scale=0.3)

# name -> (GemmCase, knob of mdm_set_gemm_variant, kernel the launch must land on)
ALIGNED = {}
ODD = {}


def _add(table, knob, kernel, **kw):
    c = GemmCase(**kw)
    assert c.name not in table
    table[c.name] = (c, knob, kernel)


for _f in ("bf16", "f16"):
    _add(ALIGNED, 0, "gemm2.hip 64-row", name=f"gemm2-64-{_f}", M=200, N=384, K=128, a_fmt=_f, precision=1, **_FULL)
    _add(ALIGNED, 0, "gemm2.hip 64-row", name=f"gemm2-64-r1mod-{_f}", M=200, N=384, K=128, a_fmt=_f, precision=1, **{**_FULL, "r1_mod": 50})
    _add(ALIGNED, 0, "gemm2.hip 128-row", name=f"gemm2-128-grouped-{_f}", M=200, N=256, K=128, a_fmt=_f, precision=1, sizes=(130, 0, 1, 69),
         gather=True, src_rows=90, **_FULL)
    _add(ALIGNED, 6, "gemm4.hip", name=f"gemm4-{_f}", M=300, N=256, K=64, a_fmt=_f, precision=1, **{**_FULL, "r1_mod": 50})
    for _knob, _kern in ((68, "gemm_stream.hip"), (63, "gemm2.hip under knob 63")):
        _add(ALIGNED, _knob, _kern, name=f"stream{_knob}-{_f}", M=50, N=256, K=512, a_fmt=_f, precision=1, out16=True, **_STREAM)
        _add(ALIGNED, _knob, _kern, name=f"stream{_knob}-only16-{_f}", M=50, N=256, K=512, a_fmt=_f, precision=1, out32=False, out16=True,
             **_STREAM)
_add(ALIGNED, 0, "gemm3.hip", name="gemm3-f32", M=200, N=256, K=64, a_fmt="f32", precision=3, outx2=True, tol32=2e-5, **{**_EPI, "act": "gelu"})
_add(ALIGNED, 0, "gemm3.hip", name="gemm3-x2rows", M=200, N=256, K=64, a_fmt="x2", precision=3, outx2=True, tol32=2e-5, **{**_EPI, "act": "gelu"})
for _p, _tol in ((1, 2e-2), (3, 2e-5)):
    for _act in ("none", "gelu", "silu", "feat"):
        _add(ALIGNED, 36, "gemm.hip", name=f"gemm-p{_p}-{_act}", M=200, N=263, K=40, a_fmt="f32", precision=_p, tol32=_tol, **{**_EPI, "act": _act})
for _knob, _kern in ((70, "gemm_stream3.hip"), (69, "gemm3.hip under knob 69")):
    for _sizes, _src in (((5,), 8), ((200, 0, 113), 104)):
        _n = "x".join(map(str, _sizes))
        _add(ALIGNED, _knob, _kern, name=f"stream3-{_knob}-{_n}-gelu", M=sum(_sizes), N=512, K=512, a_fmt="x2", precision=3, sizes=_sizes,
             gather=True, src_rows=_src, act="gelu", outx2=True, tol32=2e-5)
        _add(ALIGNED, _knob, _kern, name=f"stream3-{_knob}-{_n}-rowscale", M=sum(_sizes), N=512, K=512, a_fmt="x2", precision=3, sizes=_sizes,
             gather=True, src_rows=_src, rowscale=True, tol32=2e-5)

# odd leading dimensions and unaligned vectors: the element-wise fallbacks of gemm2.hip / gemm3.hip, and launches that knobs 6 / 68 /
# 70 cannot take and must hand to another kernel
for _lay, _N in (("odd_ldc", 256), ("odd_ldr1", 256), ("ragged", 263), ("vec_off", 256)):
    _add(ODD, 0, "gemm2.hip", name=f"gemm2-{_lay}", M=200, N=_N, K=128, a_fmt="bf16", precision=1, layout=_lay, **_FULL)
    _add(ODD, 0, "gemm3.hip", name=f"gemm3-{_lay}", M=200, N=_N, K=64, a_fmt="f32", precision=3, layout=_lay, tol32=2e-5, **{**_EPI, "act": "gelu"})
    _add(ODD, 6, "not gemm4.hip", name=f"knob6-{_lay}", M=300, N=_N, K=64, a_fmt="bf16", precision=1, layout=_lay, **{**_FULL, "r1_mod": 50})
    _add(ODD, 68, "not gemm_stream.hip", name=f"knob68-{_lay}", M=50, N=_N, K=512, a_fmt="f16", precision=1, layout=_lay, out16=True, **_STREAM)
    _N3 = 519 if _lay == "ragged" else 512
    _add(ODD, 70, "not gemm_stream3.hip", name=f"knob70-{_lay}", M=313, N=_N3, K=512, a_fmt="x2", precision=3, layout=_lay, sizes=(200, 0, 113),
         gather=True, src_rows=104, colscale=True, rowscale=True, r1=True, r1_scale=0.5, tol32=2e-5)

# which cases each switch of the emulation must be caught on
MUTANT_CASES = {
    "a_stride_k": ("gemm2-64-bf16", "gemm3-f32", "gemm3-x2rows", "gemm-p3-none", "stream68-f16", "stream3-70-200x0x113-gelu"),
    "c_stride_n": ("gemm2-64-bf16", "gemm4-bf16", "gemm3-f32", "gemm-p3-gelu", "stream68-bf16", "stream3-70-5-rowscale", "gemm2-ragged"),
    "r1_uses_ldc": ("gemm2-64-bf16", "gemm4-f16", "gemm3-f32", "gemm-p1-silu", "stream68-bf16", "gemm2-odd_ldr1", "gemm3-odd_ldc"),
    "r2_uses_ldr1": ("gemm2-64-f16", "gemm4-bf16", "gemm3-x2rows", "gemm-p3-feat", "gemm2-odd_ldr1"),
    "r1_mod_ignored": ("gemm2-64-r1mod-bf16", "gemm2-64-r1mod-f16", "gemm4-bf16", "gemm3-f32", "gemm-p3-none"),
    "c16_dense_stride": ("gemm2-64-bf16", "gemm2-128-grouped-f16", "gemm4-bf16", "stream68-only16-f16", "stream63-only16-bf16"),
    "cx2_stride_ldc": ("gemm3-f32", "gemm3-x2rows", "stream3-70-200x0x113-gelu", "stream3-69-5-gelu"),
    "quad_spill": ("gemm2-ragged", "gemm3-ragged", "knob6-ragged", "knob68-ragged", "knob70-ragged"),
    "gather_dense_row": ("gemm2-128-grouped-bf16", "gemm2-128-grouped-f16", "stream3-70-5-gelu", "stream3-70-200x0x113-rowscale", "knob70-odd_ldc"),
}
