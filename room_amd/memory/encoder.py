"""Learned-encoder embedder: a MiniLM-shaped transformer on the GPU.

The reference embeds memory text with Xenova/all-MiniLM-L6-v2 (384-dim fp32,
mean-pool + L2-normalize, src/shared/embeddings.ts:48-69). This build has no
network, so pretrained MiniLM weights cannot be fetched; the encoder here is
the same *shape* (6 layers, 384 dim, 12 heads, mean-pool + normalize) with:

  * a self-contained subword tokenizer (suffix-stripping word pieces), so
    morphological variants share pieces ("deploying" → "deploy" + "##ing");
  * piece embeddings from the deterministic hash projection (embedder.py) —
    the residual stream therefore carries a lexically meaningful base that
    the randomly-initialized contextual layers perturb only mildly (init
    std 0.02), keeping retrieval quality ≥ the hash baseline while the
    architecture is the real one;
  * order-invariant masked mean pooling (the hash baseline's bigram
    features are word-order sensitive; pooling is not);
  * a loader for real pretrained weights (safetensors state dict via
    ROOMAMD_ENCODER_WEIGHTS) that replaces the random init when available.

Forward runs in fp32 on whatever device is available (the model is tiny:
~7M params); on ROCm the Linear layers ride hipBLASLt. Output format (384-d
fp32, L2-normalized) and the SQLite blob codec are unchanged, so the HIP
vector store and hybrid fusion are untouched.

A second, opt-in forward (impl="hip" / ROOMAMD_ENCODER_IMPL=hip) computes the
same function with the same weights on the project's HIP kernels: bf16 with
f32 accumulation, the rows of all texts packed without padding, per-text
segments (ops/csrc/encoder.hip). Its result for a text does not depend on the
batch the text is in. The default implementation and its outputs are
unchanged.
"""
from __future__ import annotations

import hashlib
import math
import os
import re
from typing import Optional

import torch

from ..core.constants import EMBEDDING_DIM

_TOKEN_RE = re.compile(r"[a-z0-9]+")
# common English suffixes, longest-first (deterministic subword stemming)
_SUFFIXES = ["ations", "ation", "ities", "iness", "ingly", "ments", "ness",
             "ingly", "able", "ible", "ment", "tion", "sion", "ing", "est",
             "ers", "ies", "ed", "er", "ly", "es", "s"]


IMPLS = ("torch", "hip")
_HIP_MAX_BATCH = 256   # texts per packed hip forward (≤ 32768 rows)


def default_impl() -> str:
    """Forward implementation when MiniEncoder gets no impl argument:
    ROOMAMD_ENCODER_IMPL=torch|hip, default torch (fp32 torch ops). "hip" is
    the bf16 forward on the project's HIP kernels."""
    impl = os.environ.get("ROOMAMD_ENCODER_IMPL") or "torch"
    if impl not in IMPLS:
        raise ValueError(f"ROOMAMD_ENCODER_IMPL must be one of {IMPLS}, "
                         f"got {impl!r}")
    return impl


def tokenize(text: str, max_pieces: int = 128) -> list[str]:
    """Lowercased word pieces: stem + ##suffix when a known suffix applies
    and the stem stays ≥3 chars; long words additionally split every 8
    chars. Deterministic and self-contained (no vocab file)."""
    pieces: list[str] = []
    for w in _TOKEN_RE.findall(text.lower()):
        stem, suffix = w, None
        for suf in _SUFFIXES:
            if w.endswith(suf) and len(w) - len(suf) >= 3:
                stem, suffix = w[: len(w) - len(suf)], "##" + suf
                break
        while len(stem) > 8:
            pieces.append(stem[:8] + "~")
            stem = stem[8:]
        pieces.append(stem)
        if suffix:
            pieces.append(suffix)
        if len(pieces) >= max_pieces:
            break
    return pieces[:max_pieces]


def _piece_vector(piece: str) -> torch.Tensor:
    """Deterministic 384-dim hash projection of one piece (the lexical base
    the contextual layers refine)."""
    v = torch.zeros(EMBEDDING_DIM)
    for salt in range(4):  # 4 sparse ±1 features per piece
        h = hashlib.blake2s(f"{salt}:{piece}".encode(), digest_size=8).digest()
        idx = int.from_bytes(h[:4], "little") % EMBEDDING_DIM
        v[idx] += 1.0 if h[4] & 1 else -1.0
    return v / 2.0  # unit-ish norm (4 ±1 entries)


class MiniEncoder:
    """6-layer pre-norm transformer encoder, 384 dim, 12 heads, FFN 1536.
    Mean-pool + L2 normalize (embeddings.ts:56-62 semantics)."""

    LAYERS = 6
    HEADS = 12
    FFN = 1536

    def __init__(self, device: Optional[str] = None, seed: int = 7,
                 weights_path: Optional[str] = None,
                 impl: Optional[str] = None):
        self.impl = impl or default_impl()
        if self.impl not in IMPLS:
            raise ValueError(f"encoder impl must be one of {IMPLS}, "
                             f"got {self.impl!r}")
        self.device = torch.device(device or (
            "cuda" if torch.cuda.is_available() else "cpu"))
        if self.impl == "hip":
            # no fallback: the hip forward is HIP kernels or nothing
            if self.device.type != "cuda" or not torch.cuda.is_available():
                raise RuntimeError(
                    'MiniEncoder(impl="hip") needs a CUDA device, got '
                    f"{self.device}")
            from .. import ops
            ops._require()
        d = EMBEDDING_DIM
        gen = torch.Generator().manual_seed(seed)

        def rnd(*shape):
            return torch.empty(*shape).normal_(0, 0.02, generator=gen)

        self.layers = []
        for _ in range(self.LAYERS):
            self.layers.append({
                "norm1": torch.ones(d), "wq": rnd(d, d), "wk": rnd(d, d),
                "wv": rnd(d, d), "wo": rnd(d, d),
                "norm2": torch.ones(d), "w1": rnd(self.FFN, d),
                "w2": rnd(d, self.FFN),
            })
        self.final_norm = torch.ones(d)
        # sinusoidal positions (deterministic, scaled small so pooling stays
        # order-tolerant)
        pos = torch.arange(256).unsqueeze(1)
        div = torch.exp(torch.arange(0, d, 2) * (-math.log(10000.0) / d))
        pe = torch.zeros(256, d)
        pe[:, 0::2] = torch.sin(pos * div)
        pe[:, 1::2] = torch.cos(pos * div)
        self.pos = 0.02 * pe
        weights_path = weights_path or os.environ.get("ROOMAMD_ENCODER_WEIGHTS")
        if weights_path and os.path.exists(weights_path):
            self._load_weights(weights_path)
        self._to_device()
        self._piece_cache: dict[str, torch.Tensor] = {}
        # anisotropy correction: transformer outputs share a large common
        # direction (GELU's positive mean drifts every text the same way),
        # which flattens cosine contrast. Estimate the common mean from
        # deterministic probe texts once and center before normalizing
        # ("all-but-the-top" post-processing).
        self.mu = torch.zeros(d, device=self.device)
        probes = [" ".join(
            hashlib.blake2s(f"{i}:{j}".encode()).hexdigest()[:6]
            for j in range(12)) for i in range(24)]
        if self.impl == "hip":
            self._hip_init()
            self.mu = self._hip_forward(probes, normalize=False).mean(0)
        else:
            self.mu = self._pool(probes).mean(0).to(self.device)

    def _to_device(self) -> None:
        for layer in self.layers:
            for k in layer:
                layer[k] = layer[k].to(self.device)
        self.final_norm = self.final_norm.to(self.device)
        self.pos = self.pos.to(self.device)

    def _load_weights(self, path: str) -> None:
        """Replace random init with a user-provided safetensors state dict
        (keys: layers.<i>.{norm1,wq,wk,wv,wo,norm2,w1,w2}, final_norm)."""
        from safetensors.torch import load_file
        sd = load_file(path)
        for i, layer in enumerate(self.layers):
            for k in layer:
                key = f"layers.{i}.{k}"
                if key in sd:
                    layer[k] = sd[key].float()
        if "final_norm" in sd:
            self.final_norm = sd["final_norm"].float()

    def _rmsnorm(self, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * w

    @torch.inference_mode()
    def encode(self, texts: list[str]) -> torch.Tensor:
        """[B, 384] fp32, centered + L2-normalized."""
        if self.impl == "hip":
            if not texts:
                return torch.zeros(0, EMBEDDING_DIM)
            # chunks bound the activation buffers; a text's row does not
            # depend on its batch, so chunking changes no result
            outs = [self._hip_forward(texts[i:i + _HIP_MAX_BATCH])
                    for i in range(0, len(texts), _HIP_MAX_BATCH)]
            out = outs[0] if len(outs) == 1 else torch.cat(outs)
            return out.cpu()
        pooled = self._pool(texts).to(self.device) - self.mu
        return torch.nn.functional.normalize(pooled, dim=-1).cpu()

    @torch.inference_mode()
    def _pool(self, texts: list[str]) -> torch.Tensor:
        """Raw mean-pooled encoder output (pre-centering)."""
        return self._pool_device(texts).cpu()

    @torch.inference_mode()
    def _pool_device(self, texts: list[str]) -> torch.Tensor:
        """_pool before its copy to the host (every launch issued, no sync)."""
        d = EMBEDDING_DIM
        piece_lists = [tokenize(t) or ["<empty>"] for t in texts]
        T = max(len(p) for p in piece_lists)
        B = len(texts)
        x = torch.zeros(B, T, d)
        mask = torch.zeros(B, T)
        for b, pieces in enumerate(piece_lists):
            vecs = []
            for p in pieces:
                vec = self._piece_cache.get(p)
                if vec is None:
                    vec = _piece_vector(p)
                    if len(self._piece_cache) < 100_000:
                        self._piece_cache[p] = vec
                vecs.append(vec)
            # one stack+copy per text (per-piece __setitem__ was ~10 ms/text)
            x[b, : len(pieces)] = torch.stack(vecs)
            mask[b, : len(pieces)] = 1.0
        x = x.to(self.device) + self.pos[:T]
        mask = mask.to(self.device)
        attn_bias = (1.0 - mask).unsqueeze(1).unsqueeze(1) * -1e9  # [B,1,1,T]
        hd = d // self.HEADS
        for layer in self.layers:
            h = self._rmsnorm(x, layer["norm1"])
            q = (h @ layer["wq"].T).view(B, T, self.HEADS, hd).transpose(1, 2)
            k = (h @ layer["wk"].T).view(B, T, self.HEADS, hd).transpose(1, 2)
            v = (h @ layer["wv"].T).view(B, T, self.HEADS, hd).transpose(1, 2)
            s = (q @ k.transpose(-1, -2)) * (hd ** -0.5) + attn_bias
            a = torch.softmax(s, dim=-1) @ v
            a = a.transpose(1, 2).reshape(B, T, d)
            x = x + a @ layer["wo"].T
            h = self._rmsnorm(x, layer["norm2"])
            x = x + torch.nn.functional.gelu(h @ layer["w1"].T) @ layer["w2"].T
        x = self._rmsnorm(x, self.final_norm)
        # masked mean pool (embeddings.ts:56-62); centering+normalize in encode()
        return ((x * mask.unsqueeze(-1)).sum(1)
                / mask.sum(1, keepdim=True))

    # ---- impl="hip": bf16 weights, packed rows, the project's own kernels

    def _hip_init(self) -> None:
        """bf16 copies of the (possibly loaded) weights, q/k/v fused; the
        projections run as one-"expert" grouped GEMMs, hence the leading 1."""
        bf = torch.bfloat16

        def w(t):
            return t.to(bf).unsqueeze(0).contiguous()

        self._hip_layers = [{
            "norm1": L["norm1"].to(bf), "norm2": L["norm2"].to(bf),
            "wqkv": w(torch.cat([L["wq"], L["wk"], L["wv"]], dim=0)),
            "wo": w(L["wo"]), "w1": w(L["w1"]), "w2": w(L["w2"]),
        } for L in self.layers]
        self._hip_final_norm = self.final_norm.to(bf)
        self._hip_pos = self.pos.float().contiguous()
        self._hip_zero_mu = torch.zeros(EMBEDDING_DIM, device=self.device)
        self._hip_feat_cache: dict[str, tuple] = {}
        # per row count: (identity pair map, 16-row tile descriptors);
        # written once, read-only afterwards
        self._hip_desc: dict[int, tuple] = {}

    def _hip_tiles(self, rows: int) -> tuple:
        hit = self._hip_desc.get(rows)
        if hit is None:
            from .. import ops
            ident = torch.arange(rows, dtype=torch.int32, device=self.device)
            desc = ops.moe_build_desc_device(
                torch.zeros(rows, dtype=torch.int32, device=self.device), 1,
                bm=16)
            hit = (ident, desc)
            if len(self._hip_desc) >= 1024:
                self._hip_desc.clear()
            self._hip_desc[rows] = hit
        return hit

    def _hip_feats(self, piece: str) -> tuple:
        """The piece's four hash features as integers, (index << 1) | plus:
        the same draws as _piece_vector."""
        f = self._hip_feat_cache.get(piece)
        if f is None:
            f = piece_features(piece)
            if len(self._hip_feat_cache) < 100_000:
                self._hip_feat_cache[piece] = f
        return f

    @torch.inference_mode()
    def _hip_forward(self, texts: list[str],
                     normalize: bool = True) -> torch.Tensor:
        """[B, 384] f32 on the device: centred and L2-normalised, or with
        normalize=False the raw pooled mean (mu is estimated from it). Every
        buffer is allocated per call, so concurrent calls share only weights."""
        from .. import ops
        d = EMBEDDING_DIM
        flat: list[int] = []
        pos_ids: list[int] = []
        cu = [0]
        for t in texts:
            pieces = tokenize(t) or ["<empty>"]
            for p in pieces:
                flat.extend(self._hip_feats(p))
            pos_ids.extend(range(len(pieces)))
            cu.append(cu[-1] + len(pieces))
        R, B = cu[-1], len(texts)
        # one pinned host-to-device copy: feats | pos_ids | cu_rows
        host = torch.tensor(flat + pos_ids + cu, dtype=torch.int32).pin_memory()
        meta = host.to(self.device, non_blocking=True)
        feats = meta[:4 * R].view(R, 4)
        pos = meta[4 * R:5 * R]
        cu_dev = meta[5 * R:]
        ident, desc = self._hip_tiles(R)

        bf = dict(dtype=torch.bfloat16, device=self.device)
        x = torch.empty(R, d, **bf)          # residual, updated in place
        h = torch.empty(R, d, **bf)
        qkv = torch.empty(R, 3 * d, **bf)
        a = torch.empty(R, d, **bf)
        o = torch.empty(R, d, **bf)
        u = torch.empty(R, self.FFN, **bf)
        gemm = ops.moe_grouped_gemm_skinny
        ops.encoder_embed(x, feats, pos, self._hip_pos)
        for i, L in enumerate(self._hip_layers):
            if i == 0:
                ops.rmsnorm(h, x, L["norm1"])
            else:
                ops.fused_add_rmsnorm(h, x, o, L["norm1"])
            gemm(qkv, h, L["wqkv"], ident, desc)
            ops.encoder_attention(a, qkv, cu_dev, cu_rows_host=cu)
            gemm(o, a, L["wo"], ident, desc)
            ops.fused_add_rmsnorm(h, x, o, L["norm2"])
            gemm(u, h, L["w1"], ident, desc)
            ops.gelu_(u)
            gemm(o, u, L["w2"], ident, desc)
        ops.fused_add_rmsnorm(h, x, o, self._hip_final_norm)
        out = torch.empty(B, d, dtype=torch.float32, device=self.device)
        ops.encoder_pool(out, h, cu_dev,
                         self.mu if normalize else self._hip_zero_mu,
                         cu_rows_host=cu, normalize=normalize)
        return out


def piece_features(piece: str) -> tuple:
    """_piece_vector's four sparse features as plain integers,
    (index << 1) | (1 for +0.5, 0 for -0.5)."""
    out = []
    for salt in range(4):
        h = hashlib.blake2s(f"{salt}:{piece}".encode(), digest_size=8).digest()
        idx = int.from_bytes(h[:4], "little") % EMBEDDING_DIM
        out.append((idx << 1) | (h[4] & 1))
    return tuple(out)


_encoders: dict[str, MiniEncoder] = {}


def get_encoder() -> MiniEncoder:
    """Process-wide encoder of the implementation the environment selects
    now; one instance per implementation."""
    impl = default_impl()
    enc = _encoders.get(impl)
    if enc is None:
        enc = _encoders[impl] = MiniEncoder(impl=impl)
    return enc


def encode_texts(texts: list[str]) -> list[list[float]]:
    return get_encoder().encode(texts).tolist()
