"""Text-motion evaluator on the HIP library: the reference's three pretrained networks (datasets1/evaluator_models.py
:79-99 ``MovementConvEncoder``, :311-350 ``TextEncoderBiGRUCo``, :353-386 ``MotionEncoderBiGRUCo``) and the wrapper that
embeds texts and motions with them (``EvaluatorModelWrapper``, datasets1/evaluator.py:418-503).

The modules are parameter containers with the reference's state-dict names, so a reference ``finest.tar`` loads strict.
Their arithmetic runs on the library: every Linear and both k4 s2 p1 convolutions on ``mdm_gemm`` at precision 3
(bf16x3, fp32-grade), the GRU recurrence on ``mdm_gru_bidir``, padding / LeakyReLU / LayerNorm on the row kernels of
csrc/evaluator.hip.  There is no eager fallback."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from .ops import PackedWeight, f32_operand, gemm_desc, linear, run_gemm

PREC = L.PREC_X3  # the evaluator has one precision: fp32-grade


def _round8(n: int) -> int:
    return (n + 7) // 8 * 8


class _Packs(nn.Module):
    """Pack cache invalidated on load_state_dict and .to() (as text_head.py); subclasses fill ``_make_packs``."""

    def __init__(self):
        super().__init__()
        self._packed = None
        self.register_load_state_dict_post_hook(lambda mod, _: setattr(mod, "_packed", None))

    def _apply(self, fn, *a, **k):
        self._packed = None
        return super()._apply(fn, *a, **k)

    def packs(self):
        key = tuple((p.data_ptr(), p._version, str(p.device)) for p in self.parameters())
        if self._packed is None or self._packed[0] != key:
            L.require_cuda(*self.parameters())
            with torch.no_grad():
                self._packed = (key, self._make_packs())
        return self._packed[1]


def _lin(m: nn.Linear):
    return PackedWeight(m.weight.detach(), with_lo=True), m.bias.detach().float().contiguous()


class _BiGRUHead(_Packs):
    """The shared tail of both GRU encoders: input_emb -> bidirectional GRU -> output_net (Linear, LayerNorm, LeakyReLU,
    Linear).  ``gru`` / ``output_net`` keep nn.GRU / nn.Sequential names (``gru.weight_ih_l0_reverse``, ``output_net.3.bias``)."""

    def _init_tail(self, hidden_size: int, output_size: int):
        self.hidden_size = hidden_size
        self.gru = nn.GRU(hidden_size, hidden_size, batch_first=True, bidirectional=True)
        self.output_net = nn.Sequential(nn.Linear(hidden_size * 2, hidden_size), nn.LayerNorm(hidden_size),
                                        nn.LeakyReLU(0.2, inplace=True), nn.Linear(hidden_size, output_size))
        self.hidden = nn.Parameter(torch.randn((2, 1, hidden_size)))

    def _tail_packs(self):
        g = self.gru
        w_ih = torch.cat([g.weight_ih_l0, g.weight_ih_l0_reverse], 0).detach()  # [6H, H]: gx of both directions in one GEMM
        b_ih = torch.cat([g.bias_ih_l0, g.bias_ih_l0_reverse], 0).detach().float().contiguous()
        w_hh = torch.stack([g.weight_hh_l0, g.weight_hh_l0_reverse], 0).detach().float().contiguous()
        b_hh = torch.stack([g.bias_hh_l0, g.bias_hh_l0_reverse], 0).detach().float().contiguous()
        ln = self.output_net[1]
        return {"in": _lin(self.input_emb), "ih": (PackedWeight(w_ih, with_lo=True), b_ih), "w_hh": w_hh, "b_hh": b_hh,
                "h0": self.hidden.detach().float().reshape(2, -1).contiguous(), "o0": _lin(self.output_net[0]),
                "ln": (ln.weight.detach().float().contiguous(), ln.bias.detach().float().contiguous(), float(ln.eps)),
                "o3": _lin(self.output_net[3])}

    def _gru_tail(self, p, x: torch.Tensor, lens_host: np.ndarray) -> torch.Tensor:
        """x (B, T, H) input embeddings -> (B, output_size)."""
        B, T, H = x.shape
        gx = linear(x, *p["ih"], precision=PREC)  # (B, T, 2 * 3H) == (B, T, 2, 3H)
        lib = L.lib()
        lh = np.ascontiguousarray(lens_host, dtype=np.int32)
        ld = torch.from_numpy(lh).to(x.device)
        nbytes = lib.mdm_gru_bidir_workspace_bytes(B, H)
        ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=x.device)
        last = torch.empty(B, 2 * H, dtype=torch.float32, device=x.device)
        L.check(lib.mdm_gru_bidir(gx.data_ptr(), p["w_hh"].data_ptr(), p["b_hh"].data_ptr(), p["h0"].data_ptr(), ld.data_ptr(),
                                  lh.ctypes.data, B, T, H, last.data_ptr(), ws.data_ptr(), nbytes,
                                  L.stream_ptr()), "mdm_gru_bidir")
        y = linear(last, *p["o0"], precision=PREC)
        lw, lb, eps = p["ln"]
        L.check(lib.mdm_eval_ln_leaky(y.data_ptr(), B, H, lw.data_ptr(), lb.data_ptr(), eps, y.data_ptr(), L.stream_ptr()),
                "mdm_eval_ln_leaky")
        return linear(y, *p["o3"], precision=PREC)


def _check_lens(lens: np.ndarray, T: int, what: str):
    if lens.size and (lens.min() < 1 or lens.max() > T):
        raise L.MdmError(f"{what} must lie in [1, {T}] (got {lens.min()}..{lens.max()})")


class MovementConvEncoder(_Packs):
    """evaluator_models.py:79-99: Conv1d(k4 s2 p1) -> LeakyReLU(0.2) twice, then Linear; (B, T, C) -> (B, T // 4, out).
    Each convolution is one GEMM: the input is copied channels-last with a zero frame at each end (channels padded to a
    multiple of 8), so output frame t reads the 4 C contiguous values of padded frames 2t .. 2t + 3 (row stride 2 C),
    against the weight re-laid as W'[o, k C + c] = W[o, c, k]."""

    def __init__(self, input_size: int, hidden_size: int, output_size: int):
        super().__init__()
        self.main = nn.Sequential(nn.Conv1d(input_size, hidden_size, 4, 2, 1), nn.Dropout(0.2, inplace=True),
                                  nn.LeakyReLU(0.2, inplace=True), nn.Conv1d(hidden_size, output_size, 4, 2, 1),
                                  nn.Dropout(0.2, inplace=True), nn.LeakyReLU(0.2, inplace=True))
        self.out_net = nn.Linear(output_size, output_size)

    @staticmethod
    def _conv_pack(conv: nn.Conv1d):
        w = conv.weight.detach().float()  # [O, C, 4]
        O, Cin, _ = w.shape
        Cp = _round8(Cin)
        wr = torch.zeros(O, 4, Cp, dtype=torch.float32, device=w.device)
        wr[:, :, :Cin] = w.permute(0, 2, 1)
        return PackedWeight(wr.reshape(O, 4 * Cp), with_lo=True), conv.bias.detach().float().contiguous(), Cp

    def _make_packs(self):
        return {"c0": self._conv_pack(self.main[0]), "c3": self._conv_pack(self.main[3]), "out": _lin(self.out_net)}

    def _conv(self, src: torch.Tensor, ld_src: int, B: int, T: int, Cin: int, pk, leaky_in: bool) -> torch.Tensor:
        """k4 s2 p1 conv of rows src[(b T + t) ld_src + c] -> (B * (T // 2), O) (no activation on the output)."""
        w, bias, Cp = pk
        lib = L.lib()
        padded = torch.empty(B, T + 2, Cp, dtype=torch.float32, device=src.device)
        L.check(lib.mdm_eval_pad_rows(src.data_ptr(), ld_src, B, T, Cin, Cp, 1, int(leaky_in), padded.data_ptr(), L.stream_ptr()),
                "mdm_eval_pad_rows")
        To = T // 2
        out = torch.empty(B * To, w.N, dtype=torch.float32, device=src.device)
        d = gemm_desc(PREC)
        d.A = f32_operand(padded, 2 * Cp)
        d.A.rpg, d.A.gstride = To, (T + 2) * Cp  # row b To + t -> padded frame 2t of sample b
        d.W = w.operand()
        d.M, d.N, d.K = B * To, w.N, 4 * Cp
        d.C, d.ldc = out.data_ptr(), out.stride(0)
        d.bias = bias.data_ptr()
        run_gemm(d)
        return out

    @torch.no_grad()
    def encode(self, motions: torch.Tensor, feats: Optional[int] = None) -> torch.Tensor:
        """motions (B, T, F) on the device -> movements (B, T // 4, out), reading the first ``feats`` features of each
        frame (the wrapper passes F - 4: ``motions[..., :-4]``)."""
        L.require_cuda(motions)
        x = motions.detach().float().contiguous()
        B, T, F = x.shape
        Cin = F if feats is None else feats
        if Cin != self.main[0].in_channels:
            raise L.MdmError(f"movement encoder expects {self.main[0].in_channels} features, got {Cin}")
        if T < 4:
            raise L.MdmError("the movement encoder needs at least 4 frames")
        p = self.packs()
        h1 = self._conv(x, F, B, T, Cin, p["c0"], False)
        T1 = T // 2
        h2 = self._conv(h1, h1.shape[1], B, T1, h1.shape[1], p["c3"], True)  # LeakyReLU of conv 1 in the pad copy
        T2 = T1 // 2
        O = h2.shape[1]
        L.check(L.lib().mdm_eval_pad_rows(h2.data_ptr(), O, B, T2, O, O, 0, 1, h2.data_ptr(), L.stream_ptr()),
                "mdm_eval_pad_rows")  # LeakyReLU of conv 2, in place
        return linear(h2, *p["out"], precision=PREC).reshape(B, T2, -1)

    def forward(self, inputs):
        return self.encode(inputs)


class TextEncoderBiGRUCo(_BiGRUHead):
    """evaluator_models.py:311-350: (word_embs + pos_emb(pos_ohot)) -> input_emb -> BiGRU(H) -> output_net."""

    def __init__(self, word_size: int, pos_size: int, hidden_size: int, output_size: int, device=None):
        super().__init__()
        self.pos_emb = nn.Linear(pos_size, word_size)
        self.input_emb = nn.Linear(word_size, hidden_size)
        self._init_tail(hidden_size, output_size)

    def _make_packs(self):
        return {"pos": _lin(self.pos_emb), **self._tail_packs()}

    @torch.no_grad()
    def encode(self, word_embs: torch.Tensor, pos_ohot: torch.Tensor, cap_lens) -> torch.Tensor:
        L.require_cuda(word_embs, pos_ohot)
        w = word_embs.detach().float().contiguous()
        po = pos_ohot.detach().float().contiguous()
        B, T, _ = w.shape
        lens = np.asarray(torch.as_tensor(cap_lens).flatten().tolist(), dtype=np.int64)
        if lens.shape[0] != B:
            raise L.MdmError("one caption length per sample")
        _check_lens(lens, T, "caption lengths")
        p = self.packs()
        x = linear(po, *p["pos"], r1=w, precision=PREC)  # word_embs + pos_emb(pos_ohot)
        x = linear(x, *p["in"], precision=PREC)
        return self._gru_tail(p, x, lens)

    def forward(self, word_embs, pos_onehot, cap_lens):
        return self.encode(word_embs, pos_onehot, cap_lens)


class MotionEncoderBiGRUCo(_BiGRUHead):
    """evaluator_models.py:353-386: input_emb -> BiGRU(H) -> output_net over movements with lengths m_lens // unit."""

    def __init__(self, input_size: int, hidden_size: int, output_size: int, device=None):
        super().__init__()
        self.input_emb = nn.Linear(input_size, hidden_size)
        self._init_tail(hidden_size, output_size)

    def _make_packs(self):
        return self._tail_packs()

    @torch.no_grad()
    def encode(self, inputs: torch.Tensor, m_lens) -> torch.Tensor:
        L.require_cuda(inputs)
        x = inputs.detach().float().contiguous()
        B, T, _ = x.shape
        lens = np.asarray(torch.as_tensor(m_lens).flatten().tolist(), dtype=np.int64)
        if lens.shape[0] != B:
            raise L.MdmError("one motion length per sample")
        _check_lens(lens, T, "motion lengths (in movement units)")
        p = self.packs()
        return self._gru_tail(p, linear(x, *p["in"], precision=PREC), lens)

    def forward(self, inputs, m_lens):
        return self.encode(inputs, m_lens)


class MotionTextEvaluator(nn.Module):
    """``EvaluatorModelWrapper`` (datasets1/evaluator.py:418-503) on the HIP library.  Sub-module names follow the
    checkpoint keys: ``movement_encoder``, ``text_encoder``, ``motion_encoder``."""

    def __init__(self, dim_pose: int = 263, dim_word: int = 300, dim_pos_ohot: int = 15, dim_movement_enc_hidden: int = 512,
                 dim_movement_latent: int = 512, dim_text_hidden: int = 512, dim_motion_hidden: int = 1024,
                 dim_coemb_hidden: int = 512, unit_length: int = 4):
        super().__init__()
        self.dim_pose, self.unit_length = dim_pose, unit_length
        self.movement_encoder = MovementConvEncoder(dim_pose - 4, dim_movement_enc_hidden, dim_movement_latent)
        self.text_encoder = TextEncoderBiGRUCo(dim_word, dim_pos_ohot, dim_text_hidden, dim_coemb_hidden)
        self.motion_encoder = MotionEncoderBiGRUCo(dim_movement_latent, dim_motion_hidden, dim_coemb_hidden)
        self.epoch = None

    @classmethod
    def from_checkpoint(cls, path: str, device="cuda", **kw):
        """A reference ``finest.tar`` (keys movement_encoder / text_encoder / motion_encoder / epoch), loaded strict."""
        ckpt = torch.load(path, map_location="cpu")
        ev = cls(**kw)
        ev.movement_encoder.load_state_dict(ckpt["movement_encoder"])
        ev.text_encoder.load_state_dict(ckpt["text_encoder"])
        ev.motion_encoder.load_state_dict(ckpt["motion_encoder"])
        ev.epoch = ckpt.get("epoch")
        return ev.to(device).eval()

    @property
    def device(self):
        return self.text_encoder.hidden.device

    @staticmethod
    def align_index(m_lens) -> np.ndarray:
        """The reference's output order: ``np.argsort(m_lens.data.tolist())[::-1].copy()`` (evaluator.py:458)."""
        return np.argsort(torch.as_tensor(m_lens).flatten().tolist())[::-1].copy()

    def _motion_embed(self, motions: torch.Tensor, m_lens) -> torch.Tensor:
        """Embeddings in the caller's order (permuting rows commutes with the per-sample encoders)."""
        x = motions.detach().to(self.device).float().contiguous()
        if x.shape[-1] != self.dim_pose:
            raise L.MdmError(f"motions have {x.shape[-1]} features, the evaluator expects {self.dim_pose}")
        movements = self.movement_encoder.encode(x, feats=self.dim_pose - 4)  # motions[..., :-4] (evaluator.py:463)
        lens = torch.as_tensor(m_lens).flatten().cpu() // self.unit_length
        return self.motion_encoder.encode(movements, lens)

    @torch.no_grad()
    def get_co_embeddings(self, word_embs, pos_ohot, cap_lens, motions, m_lens):
        """(text_embedding, motion_embedding), both permuted by ``align_index(m_lens)`` like the reference."""
        idx = torch.from_numpy(self.align_index(m_lens)).to(self.device)
        mot = self._motion_embed(motions, m_lens)
        txt = self.text_encoder.encode(word_embs.detach().to(self.device), pos_ohot.detach().to(self.device), cap_lens)
        return txt.index_select(0, idx), mot.index_select(0, idx)

    @torch.no_grad()
    def get_motion_embeddings(self, motions, m_lens):
        idx = torch.from_numpy(self.align_index(m_lens)).to(self.device)
        return self._motion_embed(motions, m_lens).index_select(0, idx)
