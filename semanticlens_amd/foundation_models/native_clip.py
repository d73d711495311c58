"""NativeClip / NativeSigLip — CLIP-family foundation models whose towers run on the package's own HIP kernels.

The reference's ``OpenClip.encode_image`` / ``encode_text`` (foundation_models/clip.py:103-135) call straight
into the third-party ``open_clip`` torch model.  ``NativeClip`` wraps any such ``AbstractVLM`` (tokenizer and
preprocessing stay the wrapped object's), reads the weights out of its torch modules once, and runs the
pre-LN transformer towers through the C ABI (K11: ``sl_linear`` = fp32-input MFMA GEMM with bias / GELU /
residual / patch-scatter epilogues, ``sl_layernorm``, ``sl_attention``, ``sl_patchify``, ``sl_embed_tokens``).
``gemm="bf16x3"`` (default) runs the linear layers as split-bf16 GEMMs on the bf16 matrix cores (three MFMAs per
product, fp32 accumulate: fp32-class accuracy, ~2.4x the fp32-MFMA rate) with weights split once at construction and
activations emitted in split form by the producing kernel; ``gemm="f32"`` uses the fp32-input MFMA GEMM.  Either
way features agree with the torch modules to ~1e-5 relative, and the object plugs into ``Lens`` and
``ActivationComponentVisualizer`` like any other ``AbstractVLM``.

Module layouts read (probed by attribute; anything else is refused with a ``TypeError`` that names what was found):

* **open_clip ``CLIP``** (what ``OpenClip(url)`` builds for the ViT-B/32, B/16, L/14 ... families, clip.py:52-62):
  ``visual`` = ``VisionTransformer`` {``conv1`` (no bias), ``class_embedding``, ``positional_embedding``, ``ln_pre``
  (or Identity), ``transformer.resblocks[i]`` {``ln_1``, ``attn`` (``nn.MultiheadAttention``), ``ls_1``, ``ln_2``,
  ``mlp`` (``c_fc``, ``gelu``, ``c_proj``), ``ls_2``}, ``ln_post``, ``proj``, ``pool_type`` in {``tok``, ``avg``},
  ``final_ln_after_pool``}; text members on the model itself: ``token_embedding``, ``positional_embedding``,
  ``transformer``, ``ln_final``, ``text_projection`` (matrix or ``nn.Linear``), ``attn_mask``, ``text_pool_type`` in
  {``argmax``, ``first``, ``last``}.  LayerScale (``ls_1`` / ``ls_2`` with a ``gamma``) is folded into the weights of
  the projection it follows.  Attention pooling (CoCa) and hybrid / convolutional towers (MobileCLIP) are refused.
* **open_clip ``CLIP`` with a ResNet image tower** (``OpenClip("RN50", ...)`` — BASELINE configs[0]'s embed model; RN101, RN50x4 ...):
  ``visual`` = ``ModifiedResNet`` {three-conv stem, ``layer1..4``, ``attnpool`` = ``AttentionPool2d`` {``positional_embedding``,
  ``q_proj``, ``k_proj``, ``v_proj``, ``c_proj``, ``num_heads``}}.  The convolutional trunk stays on PyTorch (MIOpen), like a probed
  model's forward; the attention pool and the projection to the joint space run on the kernels (``NativeResNetVision``:
  ``sl_tokens_from_map``, two GEMMs, ``sl_attention_pool_q``, ``c_proj``); the text tower natively as above.
* **open_clip ``CustomTextCLIP`` with a timm trunk** (what ``SigLipV2()`` builds, clip.py:190-211,
  ``hf-hub:timm/ViT-B-16-SigLIP2``): ``visual`` = ``TimmModel`` {``trunk`` = timm ``VisionTransformer`` with
  ``patch_embed.proj`` (bias), ``pos_embed``, no class token, ``blocks[i]`` {``norm1``, ``attn.qkv`` / ``attn.proj``,
  ``norm2``, ``mlp.fc1`` / ``act`` / ``fc2``}, ``norm``, ``attn_pool`` (``AttentionPoolLatent``: ``latent``, ``q``, ``kv``,
  ``proj``, ``norm``, ``mlp``), ``head``}; ``text`` = open_clip ``TextTransformer`` (non-causal, ``pool_type="last"``,
  ``text_projection`` = ``nn.Linear`` with bias).  ``NativeSigLip``.
* **transformers ``SiglipModel``** (``vision_model`` / ``text_model``; the SigLIP-so400m geometry of BASELINE configs[3]).
  ``NativeSigLip``.
* ``synth.SyntheticClip`` (the bench's random-init ViT-B/32).

head_dim 32, 64, 72, 80, 88, 96, 104 or 128 in the towers (any multiple of 4 up to 128 in the pooling heads).  open_clip / timm are not installed in this image, so the open_clip layouts are exercised
against ``tests/openclip_like.py`` — torch modules carrying open_clip 3.0's attribute tree — and parity for this row
stays build-vs-torch-module (the reference's own tests pin shapes only, tests/foundation_models/test_clip.py:32-85).
"""
from __future__ import annotations

import torch
from torch import nn

from semanticlens_amd import _native as N
from semanticlens_amd.foundation_models.base import AbstractVLM


def _f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _first(obj, *names):
    for n in names:
        cur = obj
        ok = True
        for part in n.split("."):
            if not hasattr(cur, part):
                ok = False
                break
            cur = getattr(cur, part)
        if ok and cur is not None:
            return cur
    raise AttributeError(f"none of {names} found on {type(obj).__name__}")


_HEAD_DIMS = (32, 64, 72, 80, 88, 96, 104, 128)  # exactly csrc/encoder_attention.hip's SL_ATTENTION_HEAD_DIMS (sl_attention / sl_attention_bf16x3)


def _ln(mod: nn.Module, device):
    """(gamma, beta, eps) of a LayerNorm-like module (open_clip's ``LayerNorm`` / ``LayerNormFp32`` subclass nn.LayerNorm)."""
    if not isinstance(mod, nn.LayerNorm) or mod.weight is None or mod.bias is None:
        raise TypeError(f"expected an affine LayerNorm, found {type(mod).__name__}")
    return _f32(mod.weight, device), _f32(mod.bias, device), float(mod.eps)


def _is_identity(mod) -> bool:
    return mod is None or isinstance(mod, (nn.Identity, nn.Dropout))


def _act_code(act) -> int:
    """Activation of an MLP: a module (nn.GELU with ``approximate``, open_clip's QuickGELU, timm's GELUTanh / QuickGELU) or a
    config string (transformers: ``gelu``, ``gelu_pytorch_tanh``, ``quick_gelu``)."""
    if isinstance(act, nn.Module):
        name = type(act).__name__.lower()
        if isinstance(act, nn.GELU) and getattr(act, "approximate", "none") == "tanh":
            return N.SL_ACT_GELU_TANH
    else:
        name = (act or "gelu").lower()
    if "quick" in name:
        return N.SL_ACT_QUICKGELU
    if "tanh" in name:
        return N.SL_ACT_GELU_TANH
    if "gelu" in name:
        return N.SL_ACT_GELU
    raise TypeError(f"unsupported MLP activation {name!r} (GELU, tanh-GELU and QuickGELU are built)")


def _layer_scale(mod, device):
    """LayerScale gamma of a residual branch (open_clip ``ls_1`` / ``ls_2``, timm ``ls1`` / ``ls2``), or None."""
    if _is_identity(mod):
        return None
    gamma = getattr(mod, "gamma", None)
    if gamma is None:
        raise TypeError(f"residual-branch scale {type(mod).__name__} has no `gamma`")
    return _f32(gamma, device)


class _Layer:
    """One linear layer: ``w`` the fp32 ``(N, K)`` weight, ``b`` the fp32 bias or None, ``op`` the weight as the tower's
    arithmetic multiplies it (set by the arithmetic's ``hold``)."""

    def __init__(self, w: torch.Tensor, b: torch.Tensor | None = None):
        self.w, self.b, self.op = w, b, None

    @classmethod
    def of(cls, lin: nn.Linear, device):
        """An ``nn.Linear``; a missing bias reads as zeros."""
        b = _f32(lin.bias, device) if lin.bias is not None else torch.zeros(lin.out_features, dtype=torch.float32, device=device)
        return cls(_f32(lin.weight, device), b)

    @classmethod
    def cat(cls, lins, device):
        """Several ``nn.Linear`` over one input as one layer: weight rows and biases concatenated (``[q | k | v]``, ``[k | v]``)."""
        parts = [cls.of(lin, device) for lin in lins]
        return cls(torch.cat([p.w for p in parts]).contiguous(), torch.cat([p.b for p in parts]).contiguous())

    def scaled(self, gamma):
        """LayerScale folded into the projection it follows: gamma * (W x + b) = (gamma W) x + gamma b."""
        return self if gamma is None else _Layer((self.w * gamma[:, None]).contiguous(), (self.b * gamma).contiguous())


class _F32:
    """The towers' arithmetic under ``gemm="f32"``: weights and GEMM operands are fp32 tensors, the linear layers run on the
    fp32-input MFMA GEMM (``N.linear``), attention on ``sl_attention``.  Each step names its destination as ``out``; a step
    that is asked for ``as_operand`` leaves what the next GEMM reads — here the same fp32 tensor."""

    @staticmethod
    def hold(*layers):
        for layer in layers:
            if layer is not None:
                layer.op = layer.w

    @staticmethod
    def buffer(rows: int, cols: int, device):
        return torch.empty((rows, cols), dtype=torch.float32, device=device)

    @staticmethod
    def operand(x: torch.Tensor):
        return x

    @staticmethod
    def layernorm(x, ln, out=None):
        return N.layernorm(x, *ln, out=out)

    @staticmethod
    def linear(x, layer: _Layer, act=N.SL_ACT_NONE, residual=None, out=None, as_operand=False, scatter=None, rowadd=None):
        return N.linear(x, layer.op, layer.b, act=act, residual=residual, out=out, scatter=scatter, rowadd=rowadd)

    @staticmethod
    def attention(qkv, B, T, heads, head_dim, causal, out, as_operand=True):
        return N.attention(qkv, B, T, heads, head_dim, causal, out=out)

    @staticmethod
    def patchify(img, patch: int):
        return N.patchify(img, patch)


class _Bf16x3:
    """The towers' arithmetic under ``gemm="bf16x3"``: weights are split once (``N.Split.of``), activations leave the
    producing kernel in split form (``as_operand``: into the ``N.Split`` given as ``out``, or a fresh one), the linear layers
    run as split-bf16 x3 GEMMs (``N.linear3``) and attention as ``sl_attention_bf16x3``.  Results that are not the next
    GEMM's operand (the residual stream, qkv, pooled rows) stay fp32."""

    @staticmethod
    def hold(*layers):
        for layer in layers:
            if layer is not None and layer.op is None:
                layer.op = N.Split.of(layer.w)

    @staticmethod
    def buffer(rows: int, cols: int, device):
        return N.Split(rows, cols, device)

    @staticmethod
    def operand(x: torch.Tensor):
        return N.Split.of(x)

    @staticmethod
    def layernorm(x, ln, out=None):
        return N.layernorm(x, *ln, out_split=out if out is not None else N.Split(x.shape[0], x.shape[1], x.device))

    @staticmethod
    def linear(x, layer: _Layer, act=N.SL_ACT_NONE, residual=None, out=None, as_operand=False, scatter=None, rowadd=None):
        if as_operand:  # e.g. the GELU output leaves as split bf16
            return N.linear3(x, layer.op, layer.b, act=act, out_split=out if out is not None else N.Split(x.shape[0], layer.w.shape[0], x.buf.device))
        return N.linear3(x, layer.op, layer.b, act=act, residual=residual, out=out, scatter=scatter, rowadd=rowadd)

    @staticmethod
    def attention(qkv, B, T, heads, head_dim, causal, out, as_operand=True):
        """Both products split-bf16 x3.  ``as_operand=False``: a fresh fp32 result (``out`` is left alone), for the pooled last
        block, which splits the rows it gathers instead of the whole matrix."""
        if as_operand:
            return N.attention(qkv, B, T, heads, head_dim, causal, out_split=out, bf16x3=True)
        return N.attention(qkv, B, T, heads, head_dim, causal, bf16x3=True)

    @staticmethod
    def patchify(img, patch: int):
        B, C, Hi, Wi = img.shape
        return N.patchify(img, patch, out_split=N.Split(B * (Hi // patch) * (Wi // patch), C * patch * patch, img.device))


_ARITHMETICS = {"f32": _F32, "bf16x3": _Bf16x3}


class _BlockWeights:
    """Weights of one pre-LN residual block, whatever module layout they were read from:
    ``x += W_o attn(LN1(x) W_qkv^T) ; x += W_pr act(W_fc LN2(x))`` with the in-projection packed ``[q | k | v]``.  The
    readers below set ``ln1``, ``ln2`` and the four `_Layer` ``qkv``, ``o``, ``fc``, ``pr``."""

    def __init__(self, width: int, heads: int, act: int):
        self.width, self.heads, self.act = int(width), int(heads), act
        self.head_dim = self.width // self.heads
        if self.head_dim not in _HEAD_DIMS or self.head_dim * self.heads != self.width:
            raise ValueError(f"head_dim {self.head_dim} is not supported (built: {_HEAD_DIMS})")


def _read_mha_block(blk: nn.Module, device) -> _BlockWeights:
    """open_clip ``ResidualAttentionBlock`` (and ``synth._Block``): ``ln_1``, ``attn`` = nn.MultiheadAttention with the packed
    in-projection, ``ls_1``, ``ln_2``, ``mlp`` = (Linear, activation, Linear), ``ls_2``."""
    attn = getattr(blk, "attn", None)
    if not isinstance(attn, nn.MultiheadAttention) or attn.in_proj_weight is None or attn.in_proj_bias is None:
        raise TypeError("expected torch.nn.MultiheadAttention blocks with a packed in_proj_weight and bias")
    if hasattr(blk, "ln_1_kv") or getattr(blk, "ln_attn", None) is not None and not _is_identity(blk.ln_attn):
        raise TypeError("cross-attention / scaled-attention blocks are not built")
    linears = [m for m in blk.mlp.modules() if isinstance(m, nn.Linear)]
    others = [m for m in blk.mlp.children() if not isinstance(m, nn.Linear) and not _is_identity(m)]
    if len(linears) != 2 or len(others) != 1:
        raise TypeError("expected an MLP of Linear, activation, Linear")
    w = _BlockWeights(attn.embed_dim, attn.num_heads, _act_code(others[0]))
    w.ln1, w.ln2 = _ln(blk.ln_1, device), _ln(blk.ln_2, device)
    w.qkv = _Layer(_f32(attn.in_proj_weight, device), _f32(attn.in_proj_bias, device))
    w.o = _Layer.of(attn.out_proj, device).scaled(_layer_scale(getattr(blk, "ls_1", None), device))
    w.fc = _Layer.of(linears[0], device)
    w.pr = _Layer.of(linears[1], device).scaled(_layer_scale(getattr(blk, "ls_2", None), device))
    return w


def _read_hf_siglip_block(blk: nn.Module, heads: int, act: int, device) -> _BlockWeights:
    """transformers ``SiglipEncoderLayer``: ``layer_norm1``, ``self_attn`` with separate ``q_proj`` / ``k_proj`` / ``v_proj`` /
    ``out_proj`` (packed here into the ``[q | k | v]`` in-projection the attention kernel reads), ``layer_norm2``,
    ``mlp.fc1`` / ``mlp.fc2``."""
    a = blk.self_attn
    w = _BlockWeights(a.q_proj.in_features, heads, act)
    w.ln1, w.ln2 = _ln(blk.layer_norm1, device), _ln(blk.layer_norm2, device)
    w.qkv = _Layer.cat((a.q_proj, a.k_proj, a.v_proj), device)
    w.o, w.fc, w.pr = _Layer.of(a.out_proj, device), _Layer.of(blk.mlp.fc1, device), _Layer.of(blk.mlp.fc2, device)
    return w


def _read_timm_block(blk: nn.Module, device) -> _BlockWeights:
    """timm ``vision_transformer.Block``: ``norm1``, ``attn`` {``qkv`` (packed Linear), ``q_norm``, ``k_norm``, ``proj``,
    ``num_heads``}, ``ls1``, ``norm2``, ``mlp`` {``fc1``, ``act``, ``norm``, ``fc2``}, ``ls2``."""
    a = blk.attn
    if not isinstance(getattr(a, "qkv", None), nn.Linear) or not isinstance(getattr(a, "proj", None), nn.Linear):
        raise TypeError("expected timm Attention with packed `qkv` and `proj` Linear layers")
    if not (_is_identity(getattr(a, "q_norm", None)) and _is_identity(getattr(a, "k_norm", None))):
        raise TypeError("timm Attention with q/k normalisation is not built")
    if not _is_identity(getattr(blk.mlp, "norm", None)):
        raise TypeError("timm Mlp with an inner norm is not built")
    w = _BlockWeights(a.qkv.in_features, a.num_heads, _act_code(blk.mlp.act))
    w.ln1, w.ln2 = _ln(blk.norm1, device), _ln(blk.norm2, device)
    w.qkv = _Layer.of(a.qkv, device)
    w.o = _Layer.of(a.proj, device).scaled(_layer_scale(getattr(blk, "ls1", None), device))
    w.fc = _Layer.of(blk.mlp.fc1, device)
    w.pr = _Layer.of(blk.mlp.fc2, device).scaled(_layer_scale(getattr(blk, "ls2", None), device))
    return w


def _project(ar, pooled: torch.Tensor, layer: _Layer | None) -> torch.Tensor:
    """The tower's output projection of the pooled rows, in the arithmetic of the blocks (split mode: a (B, W) x (D, W)
    product is a few tiles, which the small-grid kernel walks in ~6 us; the fp32-MFMA kernel took 65)."""
    return pooled if layer is None else ar.linear(ar.operand(pooled), layer)


class _Tower:
    """L residual blocks over a (B*T, W) fp32 token matrix (the residual stream stays fp32 in both arithmetics)."""

    def __init__(self, blocks: list, ar):
        """``blocks``: `_BlockWeights` in execution order (built by one of the layout readers above); ``ar``: `_F32` or `_Bf16x3`."""
        if not blocks:
            raise TypeError("the tower has no residual blocks")
        self.ar, self.blocks = ar, blocks
        for b in blocks:
            ar.hold(b.qkv, b.o, b.fc, b.pr)
        self.width = self.blocks[0].width
        self.heads = self.blocks[0].heads

    def _after_attention(self, blk, x, att, h=None, hid=None):
        """``x += out_proj(att)``, then ``x += c_proj(act(c_fc(LN2(x))))``, in place on the rows ``x`` (all of them, or the
        pooled ones); ``h`` / ``hid``: operand buffers to reuse."""
        ar = self.ar
        ar.linear(att, blk.o, residual=x, out=x)
        h = ar.layernorm(x, blk.ln2, out=h)
        hid = ar.linear(h, blk.fc, act=blk.act, out=hid, as_operand=True)
        return ar.linear(hid, blk.pr, residual=x, out=x)

    def forward(self, x: torch.Tensor, B: int, T: int, causal: bool, pool_rows: torch.Tensor | None = None) -> torch.Tensor:
        """Runs the blocks over ``x`` in place.  ``pool_rows`` (B int64 row indices): only those rows of the final
        residual stream are needed (class token / end-of-text token), so the last block stops being computed for
        the other rows after its attention (keys and values still come from every token) and ``(B, W)`` is returned.
        Each GEMM row depends on its own input row only, so the pooled rows are bit-identical either way."""
        ar = self.ar
        M, W = x.shape
        qkv = torch.empty((M, 3 * W), dtype=torch.float32, device=x.device)
        h, att, hid = ar.buffer(M, W, x.device), ar.buffer(M, W, x.device), ar.buffer(M, self.blocks[0].fc.w.shape[0], x.device)
        for blk in self.blocks:
            ar.layernorm(x, blk.ln1, out=h)
            ar.linear(h, blk.qkv, out=qkv)
            if blk is self.blocks[-1] and pool_rows is not None:
                # attention's fp32 rows are gathered first and only those become an operand
                att32 = ar.attention(qkv, B, T, blk.heads, blk.head_dim, causal, out=att, as_operand=False)
                xp = N.gather_rows(x, pool_rows, check=False)
                return self._after_attention(blk, xp, ar.operand(N.gather_rows(att32, pool_rows, check=False)))
            ar.attention(qkv, B, T, blk.heads, blk.head_dim, causal, out=att)
            self._after_attention(blk, x, att, h, hid)
        return x


# ---- a batch as several chunks on several HIP streams (off by default) ---------------------------------------------------
# At B = 256 the ViT-B/32 tower's GEMMs have 150-600 tiles of 256 x 256 for 256 CUs: the out-projection and fc2 fill 59 %
# of the chip, fc1 78 % of its last round.  The samples of a batch are independent all the way through the tower (GEMM
# rows, attention per image), so the batch can be cut in SL_ENC_STREAMS chunks that each run the whole tower on a stream
# of their own, the idle CUs of one chunk's kernel running another's.  Every feature keeps its bits
# (tests/test_gpu_native_clip.py).  Measured (tools/encoder_bench.py, B = 256): 8.56 -> 8.11 ms in round 2, but 7.99 ->
# 8.25 ms once the residual epilogue stopped serialising its loads (round 3): a half batch's GEMMs are 75-300 tiles and run
# the 128 x 128 kernel (o-proj 65 us for HALF the rows against 63 us for all of them).  Default: one stream.
_SIDE_STREAMS: dict = {}


def _enc_streams() -> int:
    import os

    return max(1, min(4, int(os.environ.get("SL_ENC_STREAMS", "1"))))


def _in_chunks(fn, batch: torch.Tensor, rows_per_sample: int, min_rows: int = 4096) -> torch.Tensor:
    """``fn(batch)`` computed as ``SL_ENC_STREAMS`` (default 1 = off) chunks on side streams when every chunk still has at least
    ``min_rows`` token rows; otherwise one call on the current stream."""
    n = _enc_streams()
    B = batch.shape[0]
    if n == 1 or B < 2 * n or (B // n) * rows_per_sample < min_rows:
        return fn(batch)
    dev = batch.device
    key = (dev.index, n)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = [torch.cuda.Stream(dev) for _ in range(n)]
    cur = torch.cuda.current_stream(dev)
    outs = []
    for st, part in zip(_SIDE_STREAMS[key], batch.chunk(n)):
        st.wait_stream(cur)
        with torch.cuda.stream(st):
            part.record_stream(st)
            out = fn(part)
        out.record_stream(cur)
        outs.append(out)
    for st in _SIDE_STREAMS[key]:
        cur.wait_stream(st)
    return torch.cat(outs)


class NativeResNetVision:
    """CLIP's ResNet image towers (open_clip ``ModifiedResNet``: ``OpenClip("RN50", ...)``, BASELINE configs[0]'s embed model).
    The convolutional trunk (stem + ``layer1..4``: the user's torch modules, MIOpen) stays on PyTorch like any probed model's
    forward; what follows it runs on the package's kernels: the NCHW map becomes ``(B, HW + 1, C)`` token rows with the mean
    token in front (``sl_tokens_from_map``, positions added), ONE GEMM projects every token to ``[k | v]`` and one the mean
    tokens to the queries, ``sl_attention_pool_q`` attends with one query per image and head, and ``c_proj`` maps to the
    joint space.  Same arithmetic as ``attnpool.forward`` (multi_head_attention_forward with separate projection weights)."""

    def __init__(self, visual: nn.Module, device):
        pool = visual.attnpool
        for name in ("positional_embedding", "q_proj", "k_proj", "v_proj", "c_proj", "num_heads"):
            if not hasattr(pool, name):
                raise TypeError(f"visual.attnpool has no `{name}`: not open_clip's AttentionPool2d")
        self.visual = visual
        W = pool.q_proj.in_features
        self.heads, self.width = int(pool.num_heads), W
        self.head_dim = W // self.heads
        if self.head_dim * self.heads != W or self.head_dim % 4 or self.head_dim > 128:
            raise ValueError(f"attention pool: head_dim {self.head_dim} (a multiple of 4 up to 128)")
        self.pos = _f32(pool.positional_embedding, device)  # (HW + 1, W)
        self.kv = _Layer.cat((pool.k_proj, pool.v_proj), device)  # (2W, W): rows [k | v]
        self.q, self.c = _Layer.of(pool.q_proj, device), _Layer.of(pool.c_proj, device)
        # The head's four projections run on the fp32-MFMA GEMM (`N.linear`) in EVERY `gemm` mode.  A trunk hands the pool
        # tokens of magnitude ~20, its softmax logits are in the hundreds, and a 3-product bf16 split (per-product relative
        # error 2^-16..2^-17) then moves the attention weights by ~0.5 %: 1.1e-3 absolute on features of scale 22, 6x torch's
        # own fp32 distance from float64 (round-4 driver run).  The GEMMs are (B*50) x 4096 x 2048 at most: microseconds
        # beside the convolutional trunk, so the split buys nothing here.
        _F32.hold(self.kv, self.q, self.c)

    def trunk(self, img: torch.Tensor) -> torch.Tensor:
        """``(B, C, h, w)`` output of ``layer4`` — the model's own forward with the attention pool taken out."""
        v = self.visual
        pool, v.attnpool = v.attnpool, nn.Identity()
        try:
            return v(img)
        finally:
            v.attnpool = pool

    @torch.no_grad()
    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        img = N.to_device(img).to(next(self.visual.parameters()).dtype)
        return self.head(self.trunk(img))

    @torch.no_grad()
    def head(self, fmap: torch.Tensor) -> torch.Tensor:
        """The attention pool + projection of a ``(B, C, h, w)`` trunk output, on the kernels."""
        fmap = N.to_device(fmap).to(torch.float32).contiguous()
        B, C = fmap.shape[:2]
        T = fmap[0, 0].numel() + 1
        if C != self.width or T != self.pos.shape[0]:
            raise ValueError(f"trunk output {tuple(fmap.shape)} does not match the attention pool ({self.pos.shape[0] - 1} positions of width {self.width})")
        tokens = N.tokens_from_map(fmap, self.pos)  # (B, T, W), row 0 = mean token
        rows = tokens.reshape(B * T, C)
        kv = _F32.linear(rows, self.kv)  # (B*T, 2W)
        q = _F32.linear(tokens[:, 0].contiguous(), self.q)  # (B, W)
        pooled = N.attention_pool_q(q, kv, B, T, self.heads, self.head_dim)
        return _F32.linear(pooled, self.c)


class NativeVisionTower:
    """open_clip ``VisionTransformer`` forward (class token + learned positions, pre-LN blocks) on the kernels.  ``pool``:
    ``"tok"`` (class token) or ``"avg"`` (mean of the patch tokens); ``ln_after_pool`` = open_clip's ``final_ln_after_pool``;
    ``ln_pre`` may be absent (``no_ln_pre``), ``proj`` too."""

    def __init__(self, visual: nn.Module, blocks, device, ar, pool: str = "tok", ln_after_pool: bool = False):
        conv = visual.conv1
        if conv.bias is not None or conv.kernel_size != conv.stride:
            raise TypeError("NativeClip expects a bias-free patch embedding with stride == kernel size")
        if pool not in ("tok", "avg"):
            raise TypeError(f"visual.pool_type={pool!r}: only 'tok' and 'avg' are built")
        self.patch = conv.kernel_size[0]
        self.width = conv.out_channels
        self.patch_embed = _Layer(_f32(conv.weight.reshape(self.width, -1), device))  # (W, C*P*P)
        self.cls = _f32(visual.class_embedding, device)
        self.pos = _f32(_first(visual, "positional_embedding", "positional_embedding_v"), device)
        self.ln_pre = None if _is_identity(visual.ln_pre) else _ln(visual.ln_pre, device)
        self.ln_post = _ln(visual.ln_post, device)
        proj = getattr(visual, "proj", None)
        if proj is None:
            proj = getattr(visual, "proj_v", None)
        self.proj = _Layer(_f32(proj.t(), device)) if proj is not None else None  # features = x @ proj -> Linear weight (D, W)
        self.ar = ar
        ar.hold(self.patch_embed, self.proj)
        self.tower = _Tower([_read_mha_block(b, device) for b in blocks], ar)
        self.pool, self.ln_after_pool = pool, bool(ln_after_pool)
        self.pool_shortcut = True  # last block: out-proj / MLP for the class-token rows only (see _Tower.forward)

    @torch.no_grad()
    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        img = N.to_device(img).to(torch.float32).contiguous()
        return _in_chunks(self._encode, img, self.chunk_rows(img))

    def chunk_rows(self, img) -> int:
        """Token rows one image contributes (what `_in_chunks` sizes its split by)."""
        return (img.shape[2] // self.patch) * (img.shape[3] // self.patch) + 1

    def _encode(self, img: torch.Tensor) -> torch.Tensor:
        B = img.shape[0]
        n_patch = (img.shape[2] // self.patch) * (img.shape[3] // self.patch)
        T = n_patch + 1
        if T != self.pos.shape[0]:
            raise ValueError(f"image gives {T} tokens, positional embedding has {self.pos.shape[0]}")
        W = self.width
        x = torch.empty((B * T, W), dtype=torch.float32, device=img.device)
        # patch embedding GEMM; its epilogue scatters row (b, p) to token row b*T + 1 + p and adds pos[1 + p]
        self.ar.linear(self.ar.patchify(img, self.patch), self.patch_embed, out=x, scatter=(n_patch, T, 1), rowadd=self.pos)
        N.broadcast_row(self.cls, self.pos[0], B, T * W, x)  # token 0 = class embedding + pos[0]
        h = N.layernorm(x, *self.ln_pre) if self.ln_pre is not None else x
        if self.pool == "tok":
            # LayerNorm is per row, so ln_post before or after picking the class token gives the same bits
            if self.pool_shortcut:
                cls_rows = torch.arange(B, device=img.device, dtype=torch.int64) * T
                pooled = N.layernorm(self.tower.forward(h, B, T, causal=False, pool_rows=cls_rows), *self.ln_post)
            else:
                h = self.tower.forward(h, B, T, causal=False)
                pooled = N.layernorm(h, *self.ln_post, rows=B, x_row_stride=T * W)  # class-token rows only
        else:  # "avg": mean over the patch tokens (K2's token mean on the (B, T-1, W) view), ln_post on either side of it
            h = self.tower.forward(h, B, T, causal=False)
            if not self.ln_after_pool:
                h = N.layernorm(h, *self.ln_post)
            pooled = torch.empty((B, W), dtype=torch.float32, device=img.device)
            N.reduce_tokens(h.view(B, T, W)[:, 1:], N.SL_TOK_MEAN, 0, None, pooled)
            if self.ln_after_pool:
                pooled = N.layernorm(pooled, *self.ln_post)
        return _project(self.ar, pooled, self.proj)


class NativeTextTower:
    """open_clip text tower (``CLIP``'s flattened members or a ``TextTransformer``) on the kernels: token + position
    embeddings, pre-LN blocks (causal iff the module carries an ``attn_mask``), ``ln_final``, pooling at the end-of-text
    token (``"argmax"``: CLIP's tokenizer gives it the highest id), the first or the last position, then the projection
    (a matrix, an ``nn.Linear`` with bias, or none)."""

    def __init__(self, model: nn.Module, blocks, device, ar, pool: str = "argmax", causal: bool = True):
        if pool not in ("argmax", "first", "last"):
            raise TypeError(f"text pool_type={pool!r}: only 'argmax', 'first' and 'last' are built")
        if getattr(model, "cls_emb", None) is not None:
            raise TypeError("text towers with a learned class embedding (CoCa) are not built")
        self.table = _f32(model.token_embedding.weight, device)
        self.pos = _f32(_first(model, "positional_embedding", "positional_embedding_t"), device)
        self.ln_final = _ln(model.ln_final, device)
        proj = getattr(model, "text_projection", None)
        if proj is None:
            proj = getattr(model, "proj_t", None)
        if isinstance(proj, nn.Linear):
            self.proj = _Layer(_f32(proj.weight, device), _f32(proj.bias, device) if proj.bias is not None else None)
        else:
            self.proj = _Layer(_f32(proj.t(), device)) if proj is not None else None
        self.ar = ar
        ar.hold(self.proj)
        self.tower = _Tower([_read_mha_block(b, device) for b in blocks], ar)
        self.pool, self.causal = pool, bool(causal)
        self.truncate = True  # skip the positions after the batch's last end-of-text token (see __call__)
        self.pool_shortcut = True  # last block: out-proj / MLP for the pooled rows only

    @torch.no_grad()
    def __call__(self, tokens: torch.Tensor) -> torch.Tensor:
        tokens = N.to_device(tokens).to(torch.int64).contiguous()
        B, T = tokens.shape
        if T > self.pos.shape[0]:
            raise ValueError(f"{T} tokens exceed the text tower's context length {self.pos.shape[0]}")
        if self.pool == "argmax":
            at = tokens.argmax(dim=-1)  # end-of-text token (highest id): the position CLIP's text tower pools
            if self.truncate and self.causal and B > 0:
                # the tower is causal: position t only sees positions <= t, so nothing after the last end-of-text token of
                # the batch can reach a pooled feature.  Dropping those (padding) positions leaves every pooled value
                # bit-identical and shrinks the work from context_length to the longest prompt (one scalar readback).
                t_eff = int(at.max().item()) + 1
                if t_eff < T:
                    tokens, T = tokens[:, :t_eff].contiguous(), t_eff
        elif self.pool == "first":
            at = torch.zeros(B, dtype=torch.int64, device=tokens.device)
        else:
            at = torch.full((B,), T - 1, dtype=torch.int64, device=tokens.device)
        x = N.embed_tokens(self.table, tokens, self.pos[:T].contiguous())
        rows = torch.arange(B, device=tokens.device) * T + at
        if self.pool_shortcut:
            picked = self.tower.forward(x, B, T, causal=self.causal, pool_rows=rows)
        else:
            picked = N.gather_rows(self.tower.forward(x, B, T, causal=self.causal), rows, check=False)
        pooled = N.layernorm(picked, *self.ln_final)
        return _project(self.ar, pooled, self.proj)

    @property
    def b_proj(self):
        """The projection's bias: None for a matrix projection (``CLIP``), set for ``TextTransformer``'s ``nn.Linear``."""
        return self.proj.b if self.proj is not None else None


def _open_clip_text(model):
    """open_clip's text tower of ``model``: its members sit on the model itself (``CLIP``) or under ``.text``
    (``CustomTextCLIP``).  Returns that module and `NativeTextTower`'s arguments for it — None when it is not open_clip's
    ``TextTransformer`` layout (``transformer.resblocks``), which each caller refuses in its own words."""
    text = model.text if hasattr(getattr(model, "text", None), "transformer") else model
    if not hasattr(getattr(text, "transformer", None), "resblocks"):
        return text, None
    pool = getattr(text, "pool_type", None) or getattr(model, "text_pool_type", "argmax")
    return text, dict(blocks=text.transformer.resblocks, pool=pool, causal=getattr(text, "attn_mask", None) is not None)


def _require_clip_layout(model):
    """open_clip builds many variants behind the same attribute names.  What the native towers implement is listed in the
    module docstring; anything else is refused here instead of silently producing different features."""
    v = model.visual
    problems = []
    if getattr(v, "attn_pool", None) is not None:
        problems.append("visual.attn_pool is set (attention pooling)")
    if getattr(v, "pool_type", "tok") not in ("tok", "avg"):
        problems.append(f"visual.pool_type={getattr(v, 'pool_type', None)!r} (only 'tok' and 'avg')")
    if getattr(model, "text_pool_type", "argmax") not in ("argmax", "first", "last"):
        problems.append(f"text_pool_type={getattr(model, 'text_pool_type', None)!r} (only 'argmax', 'first', 'last')")
    if problems:
        raise TypeError("NativeClip does not implement this open_clip variant: " + "; ".join(sorted(set(problems))))


class _NativeVLM(AbstractVLM):
    """What the native wrappers share: ``base`` keeps tokenizer + preprocessing, `_read_towers` (the subclass) reads
    ``base.model`` into ``self.vision`` / ``self.text``."""

    _name = "native-"

    def __init__(self, base, device=None, gemm: str = "bf16x3", preprocess=None):
        """``preprocess``: ``None`` keeps ``base.preprocess`` (host transform, as upstream); a
        ``DevicePreprocess`` (or ``"device"`` to derive one from ``base.preprocessor``) runs resize / crop /
        normalise for the whole batch on the device (K12)."""
        if gemm not in _ARITHMETICS:
            raise ValueError("gemm must be 'bf16x3' or 'f32'")
        self.base = base
        dev = torch.device(device) if device is not None else next(base.model.parameters()).device
        if dev.type != "cuda":
            dev = N.default_device()
        self._device = dev
        base.to(dev)
        self._read_towers(base.model, dev, _ARITHMETICS[gemm])
        self.name = f"{self._name}{gemm}-" + getattr(base, "name", type(base).__name__)
        if preprocess == "device":
            from semanticlens_amd.foundation_models.preprocess import DevicePreprocess

            preprocess = DevicePreprocess.from_transform(base.preprocessor)
        self._preprocess = preprocess.to(dev) if preprocess is not None else None

    @property
    def device(self):
        return self._device

    @property
    def device_preprocess(self):
        """The ``DevicePreprocess`` behind :meth:`preprocess`, or None when ``base``'s host transform runs."""
        return self._preprocess

    def to(self, device):
        if torch.device(device).type != "cuda":
            raise N.NativeLibraryError(f"{type(self).__name__} runs on a HIP device only")
        return self

    def encode_image(self, img):
        return self.vision(img)

    def encode_text(self, tokens):
        return self.text(tokens)

    def preprocess(self, img):
        if self._preprocess is not None:
            out = self._preprocess(img)
            return out.unsqueeze(0) if out.ndim == 3 else out  # clip.py:160-162: a single image gets a batch axis
        return self.base.preprocess(img)

    def tokenize(self, txt, *args, **kwargs):
        return self.base.tokenize(txt, *args, **kwargs)


class NativeClip(_NativeVLM):
    """``AbstractVLM`` running ``base``'s CLIP towers on HIP kernels; ``base`` keeps tokenizer + preprocessing."""

    # The embed stage of the concept-DB build may hold preprocessed batches back until this many images are there: the
    # towers' GEMMs reach their rate from a few thousand rows, and an embedding does not depend on its batch (bit for bit).
    embed_accumulate = 256

    def _read_towers(self, model, dev, ar):
        visual = getattr(model, "visual", None)
        if visual is not None and hasattr(visual, "attnpool") and hasattr(visual, "layer4"):
            # CLIP ResNet (open_clip ModifiedResNet): conv trunk on PyTorch, attention pool + projection on the kernels;
            # the text tower in open_clip's layout or synth's (`model.text.blocks`)
            self.vision = NativeResNetVision(visual, dev)
            text, found = _open_clip_text(model)
            if found is not None:
                self.text = NativeTextTower(text, device=dev, ar=ar, **found)
            elif hasattr(getattr(model, "text", None), "blocks"):
                self.text = NativeTextTower(model, model.text.blocks, dev, ar)
            else:
                raise TypeError("NativeClip: CLIP-ResNet image tower with a text tower that is neither open_clip's nor synth's layout")
        elif visual is not None and hasattr(visual, "conv1") and hasattr(visual, "transformer"):
            # open_clip CLIP: `visual` is the whole image tower
            _require_clip_layout(model)
            self.vision = NativeVisionTower(visual, visual.transformer.resblocks, dev, ar, pool=getattr(visual, "pool_type", "tok"),
                                            ln_after_pool=getattr(visual, "final_ln_after_pool", False))
            text, found = _open_clip_text(model)
            if found is None:
                # e.g. open_clip's CustomTextCLIP around a Hugging Face text encoder: `.text.transformer` is an HF model
                raise TypeError(f"NativeClip reads open_clip's TextTransformer layout (`transformer.resblocks`); the text tower is "
                                f"{type(text).__name__} around {type(getattr(text, 'transformer', None)).__name__} — run this model "
                                "through its own torch modules (OpenClip without .native())")
            self.text = NativeTextTower(text, device=dev, ar=ar, **found)
        elif visual is not None and hasattr(model, "conv1") and hasattr(visual, "blocks"):
            # synth._ClipModel: embedding members on the model, block stacks in .visual / .text
            self.vision = NativeVisionTower(_SynthVisual(model), visual.blocks, dev, ar)
            self.text = NativeTextTower(model, model.text.blocks, dev, ar)
        else:
            found = type(visual).__name__ if visual is not None else "no `visual` member"
            raise TypeError(f"NativeClip reads open_clip's CLIP / VisionTransformer layout; {type(model).__name__} has {found} "
                            "(timm trunks: NativeSigLip; convolutional / hybrid towers such as MobileCLIP are not built)")


class _SynthVisual:
    """Adapter giving ``synth._ClipModel``'s image-tower members the names of open_clip's ``visual`` module."""

    def __init__(self, m):
        self.conv1, self.class_embedding = m.conv1, m.class_embedding
        self.positional_embedding = m.positional_embedding_v
        self.ln_pre, self.ln_post, self.proj = m.ln_pre, m.ln_post, m.proj_v


# ------------------------------------------------------------------------------------------------------------------
# SigLIP-layout towers (reference: foundation_models/clip.py:190-211 `SigLipV2`; BASELINE configs[3] names SigLIP-so400m)
# ------------------------------------------------------------------------------------------------------------------
class _MapHead:
    """Weights of a MAP head (one learned probe attends over all tokens, out-projection, LayerNorm + MLP residual branch):
    transformers' ``SiglipMultiheadAttentionPoolingHead`` and timm's ``AttentionPoolLatent`` are the same computation."""

    def __init__(self, probe, q: _Layer, kv: _Layer, o: _Layer, ln, fc1: _Layer, fc2: _Layer, heads: int, act: int):
        W = probe.numel()
        self.heads, self.head_dim, self.act = int(heads), W // int(heads), act
        if self.head_dim not in _HEAD_DIMS or self.head_dim * self.heads != W:
            raise ValueError(f"MAP head: head_dim {self.head_dim} is not supported (built: {_HEAD_DIMS})")
        # the probe is the same for every image: its query projection is a constant of the model
        self.q_probe = N.linear(probe.reshape(1, W).contiguous(), q.w, q.b).reshape(W).contiguous()
        self.kv, self.o, self.ln, self.fc1, self.fc2 = kv, o, ln, fc1, fc2  # kv: (2W, W), rows [k | v]

    @classmethod
    def from_transformers(cls, head: nn.Module, act: int, device):
        mha: nn.MultiheadAttention = head.attention
        W = mha.embed_dim
        ipw, ipb = _f32(mha.in_proj_weight, device), _f32(mha.in_proj_bias, device)
        return cls(_f32(head.probe, device), _Layer(ipw[:W].contiguous(), ipb[:W].contiguous()),
                   _Layer(ipw[W:].contiguous(), ipb[W:].contiguous()), _Layer.of(mha.out_proj, device), _ln(head.layernorm, device),
                   _Layer.of(head.mlp.fc1, device), _Layer.of(head.mlp.fc2, device), mha.num_heads, act)

    @classmethod
    def from_timm(cls, pool: nn.Module, device):
        """timm ``AttentionPoolLatent``: ``latent`` (1, 1, W), ``q``, ``kv`` (outputs ``[k | v]``), ``proj``, ``norm``, ``mlp``."""
        if getattr(pool, "latent_len", 1) != 1 or getattr(pool, "pos_embed", None) is not None:
            raise TypeError("timm AttentionPoolLatent with several latents or its own position embedding is not built")
        if not (_is_identity(getattr(pool, "q_norm", None)) and _is_identity(getattr(pool, "k_norm", None))):
            raise TypeError("timm AttentionPoolLatent with q/k normalisation is not built")
        if getattr(pool, "pool", "token") != "token":
            raise TypeError(f"timm AttentionPoolLatent pool={pool.pool!r}: only 'token'")
        return cls(_f32(pool.latent, device), _Layer.of(pool.q, device), _Layer.of(pool.kv, device), _Layer.of(pool.proj, device),
                   _ln(pool.norm, device), _Layer.of(pool.mlp.fc1, device), _Layer.of(pool.mlp.fc2, device), pool.num_heads,
                   _act_code(pool.mlp.act))


class NativeSigLipVision:
    """Image tower: patch embedding WITH bias, learned positions, no class token, non-causal blocks, a final LayerNorm,
    then the MAP head (``sl_attention_pool``); the pooled token is the image feature, optionally followed by a Linear
    (open_clip ``TimmModel.head.proj``)."""

    def __init__(self, conv: nn.Conv2d, pos: torch.Tensor, blocks: list, ln_post, head: _MapHead, device, ar,
                 final_proj: nn.Linear | None = None):
        if conv.kernel_size != conv.stride:
            raise TypeError("NativeSigLip expects a patch embedding with stride == kernel size")
        self.patch = conv.kernel_size[0]
        self.width = conv.out_channels
        self.patch_embed = _Layer(_f32(conv.weight.reshape(self.width, -1), device), _f32(conv.bias, device) if conv.bias is not None else None)
        self.pos = _f32(pos.reshape(-1, self.width), device)  # (n_patches, W)
        self.ar = ar
        self.tower = _Tower(blocks, ar)
        self.ln_post = ln_post
        self.head = head
        self.final = None
        if final_proj is not None:
            self.final = _Layer(_f32(final_proj.weight, device), _f32(final_proj.bias, device) if final_proj.bias is not None else None)
        # the head's GEMMs in the arithmetic of the blocks: in split mode its (B, W) products are small grids (gemm_skinny.hpp)
        ar.hold(self.patch_embed, head.kv, head.o, head.fc1, head.fc2, self.final)

    @classmethod
    def from_transformers(cls, vm: nn.Module, cfg, device, ar):
        """transformers ``SiglipVisionTransformer``: ``embeddings``, ``encoder.layers``, ``post_layernorm``, ``head``."""
        act = _act_code(getattr(cfg, "hidden_act", "gelu_pytorch_tanh"))
        blocks = [_read_hf_siglip_block(b, cfg.num_attention_heads, act, device) for b in vm.encoder.layers]
        return cls(vm.embeddings.patch_embedding, vm.embeddings.position_embedding.weight, blocks, _ln(vm.post_layernorm, device),
                   _MapHead.from_transformers(vm.head, act, device), device, ar)

    @classmethod
    def from_open_clip_timm(cls, visual: nn.Module, device, ar):
        """open_clip ``TimmModel``: ``trunk`` = timm ``VisionTransformer`` built with ``global_pool="map"``, ``head`` = the
        (possibly empty) projection ``nn.Sequential``."""
        t = visual.trunk
        problems = []
        if getattr(t, "global_pool", "map") != "map" or getattr(t, "attn_pool", None) is None:
            problems.append(f"trunk.global_pool={getattr(t, 'global_pool', None)!r} (only the MAP head 'map')")
        if getattr(t, "cls_token", None) is not None or getattr(t, "reg_token", None) is not None:
            problems.append("the trunk has class / register tokens")
        for name in ("norm_pre", "fc_norm"):
            if not _is_identity(getattr(t, name, None)):
                problems.append(f"trunk.{name} is not Identity")
        pe = t.patch_embed
        if not _is_identity(getattr(pe, "norm", None)) or not isinstance(getattr(pe, "proj", None), nn.Conv2d):
            problems.append("patch_embed is not a plain strided convolution")
        if not _is_identity(getattr(t, "head", None)):
            problems.append("trunk.head is not Identity (the classifier of the timm model)")
        final = None
        for name, m in (visual.head.named_children() if hasattr(visual, "head") else ()):
            if isinstance(m, nn.Linear) and final is None:
                final = m
            elif not _is_identity(m):
                problems.append(f"visual.head.{name} is a {type(m).__name__}")
        if problems:
            raise TypeError("NativeSigLip does not implement this timm trunk: " + "; ".join(problems))
        blocks = [_read_timm_block(b, device) for b in t.blocks]
        return cls(pe.proj, t.pos_embed, blocks, _ln(t.norm, device), _MapHead.from_timm(t.attn_pool, device), device, ar, final)

    @torch.no_grad()
    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        img = N.to_device(img).to(torch.float32).contiguous()
        return _in_chunks(self._encode, img, (img.shape[2] // self.patch) * (img.shape[3] // self.patch))

    def _encode(self, img: torch.Tensor) -> torch.Tensor:
        B = img.shape[0]
        T = (img.shape[2] // self.patch) * (img.shape[3] // self.patch)
        if T != self.pos.shape[0]:
            raise ValueError(f"image gives {T} patches, the positional embedding has {self.pos.shape[0]}")
        W = self.width
        ar, hd = self.ar, self.head
        x = torch.empty((B * T, W), dtype=torch.float32, device=img.device)
        # patch embedding GEMM (+ bias); its epilogue writes row (b, p) to token row b*T + p and adds pos[p]
        ar.linear(ar.patchify(img, self.patch), self.patch_embed, out=x, scatter=(T, T, 0), rowadd=self.pos)
        x = self.tower.forward(x, B, T, causal=False)
        kv = ar.linear(ar.layernorm(x, self.ln_post), hd.kv)
        pooled = N.attention_pool(hd.q_probe, kv, B, T, hd.heads, hd.head_dim)  # (B, W)
        res = ar.linear(ar.operand(pooled), hd.o)
        hid = ar.linear(ar.layernorm(res, hd.ln), hd.fc1, act=hd.act, as_operand=True)
        out = ar.linear(hid, hd.fc2, residual=res, out=res)
        return _project(ar, out, self.final)


class NativeSigLipText:
    """transformers ``SiglipTextTransformer``: token + position embeddings, NON-causal blocks (SigLIP pads to the context
    length and does not mask), ``final_layer_norm``, the LAST position pooled, then the ``head`` Linear (with bias)."""

    def __init__(self, tm: nn.Module, cfg, device, ar):
        self.table = _f32(tm.embeddings.token_embedding.weight, device)
        self.pos = _f32(tm.embeddings.position_embedding.weight, device)
        act = _act_code(getattr(cfg, "hidden_act", ""))
        self.tower = _Tower([_read_hf_siglip_block(b, cfg.num_attention_heads, act, device) for b in tm.encoder.layers], ar)
        self.ln_final = _ln(tm.final_layer_norm, device)
        self.head = _Layer(_f32(tm.head.weight, device), _f32(tm.head.bias, device))
        self.ar = ar
        ar.hold(self.head)

    @torch.no_grad()
    def __call__(self, tokens: torch.Tensor) -> torch.Tensor:
        tokens = N.to_device(tokens).to(torch.int64).contiguous()
        B, T = tokens.shape
        if T > self.pos.shape[0]:
            raise ValueError(f"{T} tokens exceed the {self.pos.shape[0]} positions of the text tower")
        x = N.embed_tokens(self.table, tokens, self.pos[:T].contiguous())
        rows = torch.arange(B, device=tokens.device, dtype=torch.int64) * T + (T - 1)
        picked = self.tower.forward(x, B, T, causal=False, pool_rows=rows)
        return _project(self.ar, N.layernorm(picked, *self.ln_final), self.head)


def friendly_batch(tokens: int, width: int, mlp: int, device=None, lo: int = 64, hi: int = 256) -> int:
    """Images per encoder call (``embed_accumulate``) whose token rows fill whole rounds of 256 x 256 GEMM tiles on the part.

    A GEMM of ``tm x tn`` tiles takes ``ceil(tm tn / CUs)`` rounds whatever its last round holds: SigLIP-so400m at 64 images
    (16 384 rows) runs its out-projection and fc2 (N = 1152: 5 tile columns) as 320 tiles = 2 rounds for 1.25 rounds of work
    (296 of the 411 TFLOP/s the same kernels reach at 256 images, where every GEMM is a whole number of rounds:
    ``profiles/r04_siglip_b64_kernel_stats.csv`` / ``_b256_``).  An embedding does not depend on the batch it is computed in, so
    the embed stage is free to pick the count: the one in ``[lo, hi]`` (multiples of 8) with the fewest tile rounds per image over the four
    GEMMs of a block."""
    cus = 256
    if device is not None and torch.cuda.is_available():
        cus = torch.cuda.get_device_properties(device).multi_processor_count or 256
    tns = [-(-3 * width // 256), -(-width // 256), -(-mlp // 256), -(-width // 256)]
    best, best_cost = hi, float("inf")
    for b in range(lo, hi + 1, 8):
        tm = -(-b * tokens // 256)
        cost = sum(-(-tm * tn // cus) for tn in tns) / b
        if cost < best_cost - 1e-12:
            best, best_cost = b, cost
    return best


class NativeSigLip(_NativeVLM):
    """``AbstractVLM`` running the towers of a SigLIP-layout model on HIP kernels.

    ``base.model`` is either what the reference's ``SigLipV2`` constructs (foundation_models/clip.py:190-211: open_clip's
    ``CustomTextCLIP`` — ``visual`` = ``TimmModel`` around a timm ViT trunk with a MAP head, ``text`` = open_clip's
    ``TextTransformer``, non-causal, pooled at the last position, projection with bias) or transformers' ``SiglipModel``
    (``vision_model`` / ``text_model``; the geometry of SigLIP-so400m — width 1152, head_dim 72 — is what BASELINE
    configs[3] names).  Tokenizer and host preprocessing stay ``base``'s; ``preprocess`` as for :class:`NativeClip`."""

    embed_accumulate = 64  # see NativeClip; replaced per instance in _read_towers (tile-friendly row count for the tower's geometry)

    def _read_towers(self, model, dev, ar):
        hf = hasattr(model, "vision_model") and hasattr(model, "text_model") and hasattr(model.vision_model, "head")
        oc = hasattr(model, "visual") and hasattr(model.visual, "trunk") and hasattr(model, "text") and hasattr(model.text, "transformer")
        text, found = _open_clip_text(model) if oc else (None, None)
        if not (hf or found is not None):
            raise TypeError("NativeSigLip expects transformers' SiglipModel layout (`vision_model` with a MAP `head`, `text_model`) "
                            "or open_clip's CustomTextCLIP layout (`visual.trunk` = timm ViT, `text` = TextTransformer)")
        if hf:
            self.vision = NativeSigLipVision.from_transformers(model.vision_model, model.config.vision_config, dev, ar)
            self.text = NativeSigLipText(model.text_model, model.config.text_config, dev, ar)
        else:
            self.vision = NativeSigLipVision.from_open_clip_timm(model.visual, dev, ar)
            self.text = NativeTextTower(text, device=dev, ar=ar, **found)
        self.embed_accumulate = friendly_batch(self.vision.pos.shape[0], self.vision.width, self.vision.tower.blocks[0].fc.w.shape[0], dev)


class NativeTextClip(_NativeVLM):
    """The wrapped model with its TEXT tower on the kernels and its image tower left to PyTorch — for CLIP models whose image
    tower the native classes do not read: MobileCLIP (``ClipMobile``, foundation_models/clip.py:214-247 — the reference
    tutorial's foundation model: a FastViT hybrid of re-parameterised convolutions behind open_clip's ``TimmModel``) and any
    other convolutional / hybrid tower.  ``base.model`` is open_clip's ``CustomTextCLIP`` (``text`` = ``TextTransformer``) or
    ``CLIP`` (text members on the model).  Text probing — ``Lens.text_probing``'s 10 000-prompt sweeps — runs natively;
    ``encode_image`` is ``base``'s own (the embed stage treats it like any user ``AbstractVLM``).  ``preprocess`` as for
    :class:`NativeClip`."""

    _name = "native-text-"

    def _read_towers(self, model, dev, ar):
        text, found = _open_clip_text(model)
        if found is None or not hasattr(text, "token_embedding"):
            raise TypeError(f"NativeTextClip reads open_clip's TextTransformer layout (`token_embedding`, `transformer.resblocks`, "
                            f"`ln_final`, `text_projection`); found {type(text).__name__}")
        if found["pool"] not in ("argmax", "first", "last"):
            raise TypeError(f"text pool_type={found['pool']!r} (only 'argmax', 'first', 'last')")
        self.text = NativeTextTower(text, device=dev, ar=ar, **found)

    def encode_image(self, img):
        return self.base.encode_image(img)


def native_model(base, gemm: str = "bf16x3", preprocess=None, image_tower: str = "native"):
    """The native counterpart of a wrapped open_clip / transformers model, chosen by its module layout.  ``image_tower``:
    ``"native"`` (refuse a tower the native classes do not read), ``"auto"`` (fall back to :class:`NativeTextClip` — torch image
    tower, native text tower — when only the image tower is refused), ``"torch"`` (always that)."""
    if image_tower not in ("native", "auto", "torch"):
        raise ValueError("image_tower must be 'native', 'auto' or 'torch'")
    if image_tower == "torch":
        return NativeTextClip(base, gemm=gemm, preprocess=preprocess)
    model = base.model
    try:
        if hasattr(model, "vision_model") or hasattr(getattr(model, "visual", None), "trunk"):
            return NativeSigLip(base, gemm=gemm, preprocess=preprocess)
        return NativeClip(base, gemm=gemm, preprocess=preprocess)
    except TypeError as err:
        if image_tower != "auto":
            raise
        try:
            return NativeTextClip(base, gemm=gemm, preprocess=preprocess)
        except TypeError:
            raise err from None
