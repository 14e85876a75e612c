"""Hand-scheduled forward/backward of the VTP towers on the gfx950 kernels (no autograd inside).

Data layout in HBM (one GPU, per tower):
  * residual stream   f32  [B*N, D]   (token-major; encoder N = 1 + hw with the cls row first, decoder N = hw)
  * GEMM operands     bf16 [rows, K]  K-contiguous; weights are bf16 copies (W and W^T) of the fp32 masters
  * qkv               bf16 [B*N, 3D]  packed exactly like attention.py:115 (q | k | v, head-major inside each);
                                      RoPE is applied in place, attention reads it with strides (no head transposes)
  * saved for backward per block: x_in f32, xn1/xn2 bf16, (mean,rstd) f32, qkv bf16, o bf16, lse f32, x_mid f32,
    x12 bf16 [M,2H] (SwiGLU pre-activations, 8|8 interleaved), hidden bf16 [M,H]  (~28 MB/image-batch-row for VTP-B;
    288 GB of HBM3E makes recomputation pointless at these sizes)
  * master params / grads: two flat f32 buffers (one fused AdamW launch, contiguous gradient buckets for RCCL).

Reference call stack this replaces: SelfAttentionBlock._forward_list (block.py:290-296) ->
SelfAttention.forward (attention.py:91-126) / SwiGLUFFN.forward (ffn.py:77-81), and their autograd backward.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from . import ops
from .ops import EPI_BF16, EPI_F32, EPI_F32_SLAB, EPI_GELU, EPI_SWIGLU
from .wgrad import Problem, plan_block


# =====================================================================================================================
# parameters: flat fp32 masters + flat fp32 grads + bf16 compute copies refreshed by ONE batched kernel
# =====================================================================================================================
class Lin:
    """Compute-side record of one linear map y = x W^T + b  (W fp32 master [N,K]).  w32: the fp32 master as [N,K]; wTs: bf16
    (gamma (.) W)^T, the dgrad operand when a LayerScale follows the linear (refreshed by a prep hook)."""
    __slots__ = ("N", "K", "w", "wT", "bias", "gw", "gb", "w32", "wTs")


class SwiGLULin:
    """w1/w2 of SwiGLUFFN fused into one interleaved [2H, D] matrix (16-row groups = 8 rows w1 | 8 rows w2)."""
    __slots__ = ("H", "K", "w12", "w12T", "b12", "gw1", "gb1")


def _flat_order(names: List[str]) -> List[str]:
    """Registration order, except that (w1.weight, w2.weight) and (w1.bias, w2.bias) are made adjacent (the SwiGLU
    wgrad / bias-grad kernels de-interleave into `w1 | w2` with a single base pointer)."""
    out, seen = [], set()
    for n in names:
        if n in seen:
            continue
        if n.endswith("mlp.w1.weight") or n.endswith("mlp.w1.bias"):
            sib = n.replace("mlp.w1.", "mlp.w2.")
            out += [n, sib]
            seen.update((n, sib))
        else:
            out.append(n)
            seen.add(n)
    return out


class ParamStore:
    def __init__(self, module: torch.nn.Module, device: torch.device):
        self.device = device
        params = dict(module.named_parameters())
        order = _flat_order(list(params.keys()))
        self.offsets: Dict[str, Tuple[int, int]] = {}
        off = 0
        for n in order:
            k = params[n].numel()
            self.offsets[n] = (off, k)
            off += (k + 3) // 4 * 4
        self.numel = off
        self.flat_p = torch.zeros(off, dtype=torch.float32, device=device)
        self.flat_g = torch.zeros(off, dtype=torch.float32, device=device)
        self.params = params
        with torch.no_grad():
            for n in order:
                o, k = self.offsets[n]
                prm = params[n]
                view = self.flat_p[o:o + k].view(prm.shape)
                view.copy_(prm.detach().to(device=device, dtype=torch.float32))
                prm.data = view
                prm.grad = self.flat_g[o:o + k].view(prm.shape)
        self._descs: List[List[int]] = []
        self._bf16_elems = 0
        self._bf16_allocs: List[Tuple[object, str, int, tuple]] = []
        self._f32_extra: List[Tuple[object, str, int]] = []
        self._desc_dev = None
        self._tiles = 0
        self._keep = []

    # ---- views
    def p(self, name: str) -> torch.Tensor:
        o, k = self.offsets[name]
        return self.flat_p[o:o + k]

    def g(self, name: str) -> torch.Tensor:
        o, k = self.offsets[name]
        return self.flat_g[o:o + k]

    def has(self, name: str) -> bool:
        return name in self.offsets

    # ---- registration of compute copies (finalize() allocates them in one flat bf16 buffer)
    def _want_bf16(self, obj, attr, n_elems, shape):
        self._bf16_allocs.append((obj, attr, self._bf16_elems, shape))
        self._bf16_elems += (n_elems + 7) // 8 * 8

    def lin(self, wname: str, bname: Optional[str], N: int, K: int, need_T: bool = True) -> Lin:
        L = Lin()
        L.N, L.K = N, K
        assert self.offsets[wname][1] == N * K, (wname, N, K)
        L.bias = self.p(bname) if bname and self.has(bname) else None
        L.gw = self.g(wname)
        L.gb = self.g(bname) if bname and self.has(bname) else None
        L.wT = None
        L.w32, L.wTs = self.p(wname).view(N, K), None
        self._want_bf16(L, "w", N * K, (N, K))
        if need_T:
            self._want_bf16(L, "wT", N * K, (K, N))
        self._descs.append(["lin", L, wname, need_T])
        return L

    def swiglu(self, prefix: str, H: int, K: int) -> SwiGLULin:
        S = SwiGLULin()
        S.H, S.K = H, K
        o1, k1 = self.offsets[prefix + "w1.weight"]
        o2, _ = self.offsets[prefix + "w2.weight"]
        assert o2 == o1 + k1 and k1 == H * K
        ob1, kb1 = self.offsets[prefix + "w1.bias"]
        ob2, _ = self.offsets[prefix + "w2.bias"]
        assert ob2 == ob1 + kb1 and kb1 == H
        S.gw1 = self.flat_g[o1:o1 + 2 * k1]
        S.gb1 = self.flat_g[ob1:ob1 + 2 * H]
        self._want_bf16(S, "w12", 2 * H * K, (2 * H, K))
        self._want_bf16(S, "w12T", 2 * H * K, (K, 2 * H))
        self._descs.append(["swiglu", S, prefix])
        return S

    def finalize(self):
        self.flat_bf16 = torch.zeros(max(self._bf16_elems, 8), dtype=torch.bfloat16, device=self.device)
        for obj, attr, off, shape in self._bf16_allocs:
            n = shape[0] * shape[1]
            setattr(obj, attr, self.flat_bf16[off:off + n].view(shape))
        rows, tiles = [], 0
        self._desc_src = []  # flat-buffer offset of each record's (first) fp32 source: which gradient bucket refreshes it (desc_runs)

        def add(src, src2, dst, dstT, R, C, mode, name):
            nonlocal tiles
            rows.append([src, src2, dst, dstT, R, C, mode, tiles])
            self._desc_src.append(self.offsets[name][0])
            tiles += (R + 255) // 256 if mode == 2 else ((R + 63) // 64) * ((C + 63) // 64)

        for d in self._descs:
            if d[0] == "lin":
                _, L, wname, need_T = d
                add(self.p(wname).data_ptr(), 0, L.w.data_ptr(), L.wT.data_ptr() if need_T else 0, L.N, L.K, 0, wname)
            else:
                _, S, prefix = d
                b12 = torch.zeros(2 * S.H, dtype=torch.float32, device=self.device)
                S.b12 = b12
                self._keep.append(b12)
                add(self.p(prefix + "w1.weight").data_ptr(), self.p(prefix + "w2.weight").data_ptr(), S.w12.data_ptr(),
                    S.w12T.data_ptr(), 2 * S.H, S.K, 1, prefix + "w1.weight")
                add(self.p(prefix + "w1.bias").data_ptr(), self.p(prefix + "w2.bias").data_ptr(), b12.data_ptr(), 0,
                    2 * S.H, 1, 2, prefix + "w1.bias")
        self._desc_dev = torch.tensor(rows, dtype=torch.int64, device=self.device)
        self._ndesc = len(rows)
        self._tiles = tiles
        self._desc_tile0 = [r[-1] for r in rows] + [tiles]  # (a record's last slot: its first tile)
        self.prep()

    def prep(self):
        """Refresh every bf16 compute copy from the fp32 masters (one kernel launch)."""
        ops.prep_weights(self._desc_dev, self._ndesc, self._tiles)
        for hook in getattr(self, "prep_hooks", ()):
            hook()
        self._prepped_version = self.flat_p._version

    def desc_runs(self, ranges):
        """runs [d0, d1) of the weight-refresh table whose fp32 sources lie in the given flat ranges (the layers of a gradient bucket)"""
        hit = [i for i, o in enumerate(self._desc_src) if any(lo <= o < hi for lo, hi in ranges)]
        runs = []
        for i in hit:
            if runs and runs[-1][1] == i:
                runs[-1][1] = i + 1
            else:
                runs.append([i, i + 1])
        return [tuple(r) for r in runs]

    def prep_runs(self, runs):
        """refresh the bf16 compute copies of the table runs only (one launch per run): the per-bucket optimizer lane of the trainer"""
        for d0, d1 in runs:
            ops.prep_weights_range(self._desc_dev[d0:], d1 - d0, self._desc_tile0[d0], self._desc_tile0[d1] - self._desc_tile0[d0])

    def mark_prepped(self, done=()):
        """every compute copy is current (the trainer refreshed them bucket by bucket): the derived-weight hooks that did not ride
        along with a bucket (`done`) + the version stamp"""
        for hook in getattr(self, "prep_hooks", ()):
            if hook not in done:
                hook()
        self._prepped_version = self.flat_p._version

    def ensure_fresh(self):
        if self.flat_p._version != self._prepped_version:
            self.prep()

    def zero_grad(self):
        self.flat_g.zero_()

    def sync_grad_views(self):
        """Every parameter's .grad must be its slice of the flat gradient buffer (the engines accumulate there).  A torch
        optimizer's zero_grad(set_to_none=True) drops the views: re-attach them, zeroed ("None" means a fresh gradient)."""
        for n, prm in self.params.items():
            if prm.grad is None and prm.requires_grad:
                o, k = self.offsets[n]
                view = self.flat_g[o:o + k].view(prm.shape)
                view.zero_()
                prm.grad = view


# =====================================================================================================================
# buffers
# =====================================================================================================================
class Workspace:
    """Named device buffers, allocated once per (name, shape, dtype) and reused every step (static memory plan)."""

    def __init__(self, device):
        self.device = device
        self._bufs: Dict[tuple, torch.Tensor] = {}
        self.wgrad_groups: Dict[tuple, object] = {}  # Stack.backward: the planned grouped weight-gradient launches over these buffers

    def get(self, name: str, shape, dtype, zero: bool = False) -> torch.Tensor:
        key = (name, tuple(shape), dtype)
        t = self._bufs.get(key)
        if t is None:
            t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.device)
            self._bufs[key] = t
        return t

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self._bufs.values())


BF, F32 = torch.bfloat16, torch.float32


def _env_flag(name: str, default: str = "1") -> bool:
    return os.environ.get(name, default) not in ("0", "false", "off")


class Overlap:
    """Side HIP streams for work that is independent of the main stream's next kernels and fills the CUs their tails leave
    idle: the weight-gradient branch of every linear backward (column sums + split-K TN GEMM + slab reduce run concurrently
    with the dgrad GEMM), the EMA teacher's forward, and -- on lane 1 -- the text tower, which the trainer issues on its own
    stream with its own wgrad side stream.  fork/join are event waits (parallel hipGraph branches under stream capture)."""

    enabled = _env_flag("VTP_OVERLAP")  # VTP_OVERLAP=0: everything in-line on one stream (clean per-kernel profiles)

    def __init__(self):
        self._sides = {}
        self._lane = 0
        self._deferred = []

    @property
    def side(self):
        return self._sides.get(self._lane)

    def _side(self):
        if self._lane not in self._sides:
            self._sides[self._lane] = torch.cuda.Stream()
        return self._sides[self._lane]

    def fork(self):
        self._side().wait_stream(torch.cuda.current_stream())

    def join(self):
        self.run_deferred()
        if self.side is not None:
            torch.cuda.current_stream().wait_stream(self.side)

    # Launch order inside a captured segment decides which hardware queue a kernel replays on: the HIP graph executor walks the
    # segment's root nodes in capture order, hands each root the next queue and lets a node inherit the queue of the first
    # predecessor that reaches it.  A side branch captured in FRONT of the main stream's first kernel therefore takes the main
    # chain's join nodes onto its own queue, and the main chain pays a cross-queue signal (10-20 us of idle chip) on the way in and
    # out of every such node.  Side work is therefore forked where its inputs are ready but ISSUED behind the main stream's next
    # kernel: defer(fn) queues the issue, run_deferred() -- called by Stack.backward behind the first dgrad GEMM of a block, and by
    # whoever joins -- performs it.
    def defer(self, fn):
        self._deferred.append(fn)

    def run_deferred(self):
        while self._deferred:
            self._deferred.pop(0)()

    def lane(self, k: int):
        """context: fork / join / side refer to side stream k while a second tower is being issued on another stream"""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            prev, self._lane = self._lane, k
            try:
                yield
            finally:
                self._lane = prev
        return ctx()


OVERLAP = Overlap()
# Decided by same-box A/B runs of rounds 1-3: apply_rope in the qkv GEMM's epilogue, the SwiGLU backward in the w3 dgrad's epilogue,
# weight gradients as TN GEMMs straight from the activation layouts (no transposed copies, no fp32 atomics from the MFMA epilogue:
# 285 vs 572 images/s), bias-gradient column sums beside (not inside) the per-layer wgrad GEMMs.  The four weight gradients of a
# transformer block are ONE grouped launch with the split-K combine and the bias-gradient column sums inside it (ops.WgradGroup),
# issued one block late so that it runs beside the NEXT block's dgrad / attention kernels (Stack.backward); the per-layer path --
# one split-K GEMM + slab reduce + column-sum launch per linear layer, beside that layer's dgrad -- is what LayerScale, stochastic
# depth and tiny token counts use.


def linear_bwd(ws: Workspace, tag: str, L, dy_b, x_b, M: int, d_in, *, need_dx: bool = True, dy_remap=(0, 0),
               x_remap=(0, 0), dx_remap=(0, 0), gw=None, gb=None, N=None, K=None, wT=None, swiglu_h: int = 0,
               bias_grad_done: bool = False, ls=None, dgrad_swiglu=None, defer=None, m_rows=None):
    """Backward of y[M,N] = x[M,K] W^T + b given dy (bf16 [M,N]):  dW += dy^T x,  db += colsum(dy),  dx = dy W.
    dx is an NT GEMM against the cached transposed weight W^T.  dW is a TN GEMM (ops.gemm_tn) straight from the activation layouts --
    no transposed copies; the transpose happens in the kernel's LDS reads -- split-K over the token dimension: slices write private
    fp32 slabs (plain stores) that one reduce kernel folds into the flat gradient; db is a column-sum launch beside it.  With `defer`
    (the transformer blocks) the problem is only recorded and the caller runs the block's weight gradients as ONE grouped launch
    (ops.WgradGroup: the 8-phase kernel, or the one-wave-per-SIMD kernel on a work-item list; K slices combined inside the launch,
    column sums fused).  m_rows (int32 [1] on the device; packed text captions): only the first m_rows[0] of the M token rows hold data --
    the dgrad runs under that row limit and the recorded weight-gradient problem sums over those rows alone (grouped launches only)."""
    if m_rows is not None and (defer is None or ls is not None or dgrad_swiglu is not None):
        raise ValueError("linear_bwd: a device row limit needs the grouped weight-gradient path (defer) and a plain dgrad")
    if L is not None:
        N = L.N if N is None else N
        K = L.K if K is None else K
        gw = L.gw if gw is None else gw
        gb = L.gb if gb is None else gb
        wT = L.wT if wT is None else wT
    c_remap = (-1, swiglu_h) if swiglu_h else (0, 0)

    def wgrad(dst, accumulate: bool, colsum=None, in_gemm: bool = False):
        """dst[N, K] (+)= dy[M, N]^T x[M, K] straight from the activation layouts (LDS transpose reads inside the GEMM), split-K into slabs;
        colsum (f32 [N]) += the column sums of dy, by a column-sum launch beside the GEMM or (in_gemm) by the GEMM itself"""
        if colsum is not None and not in_gemm:
            ops.colsum_bf16(dy_b, dy_b.stride(0), colsum, M, N, swiglu_h=swiglu_h, in_remap=dy_remap)
        kw = dict(M=N, N=K, K=M, lda=dy_b.stride(0), ldb=x_b.stride(0), ldc=K, a_remap=dy_remap, b_remap=x_remap, c_remap=c_remap,
                  a_colsum=colsum if in_gemm else None)
        St, n_el = ops.gemm_tn_splits(N, K, M), N * K  # tile-configuration aware (8-phase 256x256 kernel: tiles x splits = 256 CUs)
        if St == 1:
            ops.gemm_tn(dy_b, x_b, dst, resid=dst if accumulate else None, epi=EPI_F32, **kw)
        else:
            slab = ws.get("T.slab", (St * n_el,), F32)
            ops.gemm_tn(dy_b, x_b, slab, ldc2=n_el // 4, epi=EPI_F32_SLAB, splits=St, **kw)
            ops.reduce_slabs(slab, n_el, St, dst, n_el, accumulate=accumulate)

    if ls is not None:
        # y = gamma (.) (x W^T + b) (LayerScale, misc.py:24-25) and dy_b is the gradient of y: the branch output f is not stored
        # -- G = dy^T x and cs = colsum(dy) give dW = gamma (.) G, db = gamma (.) cs, dgamma = rowsum(W (.) G) + b (.) cs
        gamma, g_gamma = ls
        assert L is not None and not swiglu_h and dy_remap == (0, 0) and x_remap == (0, 0)
        cs = ws.get("T.ls_cs", (N,), F32).zero_()
        G = ws.get("T.ls_G", (N * K,), F32)
        OVERLAP.join()
        wgrad(G, False, cs, in_gemm=True)
        ops.layerscale_wgrad(G, L.w32, L.bias, cs, gamma, gw, gb, g_gamma, N, K)
        if need_dx:
            ops.gemm_nt(dy_b, L.wTs, d_in, M=M, N=K, K=N, lda=dy_b.stride(0), ldb=N, ldc=d_in.stride(0), epi=EPI_BF16,
                        c_remap=dx_remap)
        return
    if bias_grad_done:  # the kernel that produced dy_b already accumulated its column sums into the bias gradient
        gb = None
    if defer is not None:  # grouped weight gradients: record the problem, the caller launches the block's group later
        assert dy_remap == (0, 0) and x_remap == (0, 0)
        defer.append(Problem(dy=dy_b, x=x_b, gw=gw, gb=gb, N=N, K=K, swiglu_h=swiglu_h, Ktok=M))
    elif OVERLAP.enabled and need_dx:
        OVERLAP.join()   # previous layer's dW branch is done with the shared T.* scratch (and with its inputs)
        OVERLAP.fork()   # the side stream sees dy_b / x_b complete
        with torch.cuda.stream(OVERLAP.side):
            wgrad(gw, True, gb)
    else:
        OVERLAP.join()
        wgrad(gw, True, gb)
    if need_dx and dgrad_swiglu is not None:
        # this linear is the w3 of a SwiGLU FFN: the dgrad GEMM's epilogue applies the activation backward with the saved x12 and
        # writes dx12 directly (d_in = the [M, 2K] pre-activation gradient); dh never exists in HBM
        assert dy_remap == (0, 0) and dx_remap == (0, 0)
        ops.gemm_dgrad_swiglu(dy_b, wT, dgrad_swiglu, d_in, M, K, N)
    elif need_dx:
        ops.gemm_nt(dy_b, wT, d_in, M=M, N=K, K=N, lda=dy_b.stride(0), ldb=N, ldc=d_in.stride(0), epi=EPI_BF16,
                    a_remap=dy_remap, c_remap=dx_remap, m_rows=m_rows)


# =====================================================================================================================
# a run of SelfAttentionBlocks (block.py:137-308) -- shared by the ViT trunk and the pixel decoder
# =====================================================================================================================
class BlockW:
    pass


class BlockSaved(NamedTuple):
    """What the backward of one block reads, kept by the training forward.  attn_in / ffn_in are the inputs of norm1 / norm2: the
    block input x_in and x_mid in the plain pass, the gathered rows xs1 / xs2 of the kept images under stochastic depth."""
    attn_in: torch.Tensor   # f32 [M, D]
    xn1: torch.Tensor       # bf16 [M, D]
    st1: torch.Tensor       # f32 [M, 2] (mean, rstd)
    qkv: torch.Tensor       # bf16 [M, 3D] (RoPE applied)
    o: torch.Tensor         # bf16 [M, D]
    lse: torch.Tensor       # f32 [M * heads]
    ffn_in: torch.Tensor    # f32 [M, D]
    xn2: torch.Tensor       # bf16 [M, D]
    st2: torch.Tensor       # f32 [M, 2]
    pre: torch.Tensor       # bf16 [M, 2H] (SwiGLU, 8|8 interleaved) or [M, H] (GELU): the FFN pre-activations
    hid: torch.Tensor       # bf16 [M, H]
    # tail rows (the last block of a pass with a row plan, Stack.forward): ffn_in .. hid above have Mc rows, o keeps all M rows for the
    # attention backward, and these two are set
    o_c: Optional[torch.Tensor] = None      # bf16 [Mc, D]: the rows of o the projection ran on
    row_map: Optional[torch.Tensor] = None  # int32 [M]: full row -> compact row, -1 where nothing reads the row


ATTN_SCALE = 1.0 / math.sqrt(64.0)  # head_dim 64


# parameter names per block style (reference module trees: block.py:159-187 SelfAttentionBlock, block.py:382-399
# ResidualAttentionBlock + nn.MultiheadAttention)
_NAMES = {
    "vit": dict(n1="norm1", n2="norm2", qkv_w="attn.qkv.weight", qkv_b="attn.qkv.bias", proj_w="attn.proj.weight",
                proj_b="attn.proj.bias", ls1="ls1.gamma", ls2="ls2.gamma"),
    "text": dict(n1="ln_1", n2="ln_2", qkv_w="attn.in_proj_weight", qkv_b="attn.in_proj_bias",
                 proj_w="attn.out_proj.weight", proj_b="attn.out_proj.bias", ls1="ls_1.gamma", ls2="ls_2.gamma"),
}


class RowPlan(NamedTuple):
    """packed captions of one segment (Stack.varlen): sequence b is the rows [cu[b], cu[b + 1]) of every token buffer and only the first
    rows[0] rows hold data"""
    cu: torch.Tensor    # int32 [B + 1], device
    rows: torch.Tensor  # int32 [1], device


class Stack:
    """A run of pre-norm transformer blocks.  style "vit": SelfAttentionBlock (RoPE attention + SwiGLU FFN);
    style "text": CLIP ResidualAttentionBlock (causal attention, no RoPE, LayerNorm eps 1e-5, erf-GELU MLP of width H)."""

    def __init__(self, store: ParamStore, prefix: str, depth: int, D: int, heads: int, H: int, norm: str,
                 style: str = "vit", ffn: str = "swiglu"):
        self.store, self.depth, self.D, self.heads, self.H, self.style = store, depth, D, heads, H, style
        # FFN of the blocks: SwiGLUFFN (w1 | w2 fused + w3) or the erf-GELU MLP -- `mlp.fc1 / fc2` in ViT blocks with ffn_layer = "mlp"
        # (ffn.py:21-48), `mlp.c_fc / c_proj` in the text tower
        self.swiglu = style == "vit" and ffn != "mlp"
        self.quick_gelu = False  # GELU MLPs: QuickGELU instead of erf-GELU (text_quick_gelu; set by the owner)
        self.kind = ops.NORM_RMS if norm == "rmsnorm" else ops.NORM_LN
        if style == "text":
            self.eps = 1e-5  # nn.LayerNorm default (normalization.py:25-31)
        else:
            self.eps = 1e-5 if norm == "rmsnorm" else 1e-6  # RMSNorm default / partial(nn.LayerNorm, eps=1e-6)
        self.causal = style == "text"
        nm = _NAMES[style]
        self.blocks: List[BlockW] = []
        for i in range(depth):
            b = BlockW()
            pre = f"{prefix}{i}."
            b.n1w, b.gn1w = store.p(pre + nm["n1"] + ".weight"), store.g(pre + nm["n1"] + ".weight")
            b.n2w, b.gn2w = store.p(pre + nm["n2"] + ".weight"), store.g(pre + nm["n2"] + ".weight")
            if self.kind == ops.NORM_LN:
                b.n1b, b.gn1b = store.p(pre + nm["n1"] + ".bias"), store.g(pre + nm["n1"] + ".bias")
                b.n2b, b.gn2b = store.p(pre + nm["n2"] + ".bias"), store.g(pre + nm["n2"] + ".bias")
            else:
                b.n1b = b.gn1b = b.n2b = b.gn2b = None
            b.qkv = store.lin(pre + nm["qkv_w"], pre + nm["qkv_b"], 3 * D, D)
            b.proj = store.lin(pre + nm["proj_w"], pre + nm["proj_b"], D, D)
            if self.swiglu:
                b.w12 = store.swiglu(pre + "mlp.", H, D)
                # the fp32 forward multiplies by the masters themselves: w1 and w2 as two operands of one launch, nothing derived
                b.w1_32, b.w2_32 = store.p(pre + "mlp.w1.weight").view(H, D), store.p(pre + "mlp.w2.weight").view(H, D)
                b.b1_32, b.b2_32 = store.p(pre + "mlp.w1.bias"), store.p(pre + "mlp.w2.bias")
                b.w3 = store.lin(pre + "mlp.w3.weight", pre + "mlp.w3.bias", D, H)
            else:
                n1, n2 = ("fc1", "fc2") if style == "vit" else ("c_fc", "c_proj")
                b.fc = store.lin(f"{pre}mlp.{n1}.weight", f"{pre}mlp.{n1}.bias", H, D)
                b.w3 = store.lin(f"{pre}mlp.{n2}.weight", f"{pre}mlp.{n2}.bias", D, H)
            b.ls1 = store.p(pre + nm["ls1"]) if store.has(pre + nm["ls1"]) else None  # LayerScale (misc.py:7-26; text: block.py:388,399)
            b.ls2 = store.p(pre + nm["ls2"]) if store.has(pre + nm["ls2"]) else None
            b.gls1 = store.g(pre + nm["ls1"]) if b.ls1 is not None else None
            b.gls2 = store.g(pre + nm["ls2"]) if b.ls2 is not None else None
            # QK normalisation (attention.py:67-68): RMSNorm(head_dim) weights of q and k, shared by the heads
            qn = pre + "attn.q_norm.weight"
            if store.has(qn):
                b.qn_w, b.kn_w = store.p(qn), store.p(pre + "attn.k_norm.weight")
                b.g_qn, b.g_kn = store.g(qn), store.g(pre + "attn.k_norm.weight")
            else:
                b.qn_w = b.kn_w = b.g_qn = b.g_kn = None
            for L, gam in ((b.proj, b.ls1), (b.w3, b.ls2)):
                if gam is not None:  # dgrad operand (gamma (.) W)^T, refreshed with the other bf16 copies
                    L.wTs = torch.empty(L.K, L.N, dtype=BF, device=store.device)
                    if not hasattr(store, "prep_hooks"):
                        store.prep_hooks = []
                    store.prep_hooks.append(lambda L=L, gam=gam: ops.scaled_transpose(L.w32, gam, L.wTs, L.N, L.K))
            self.blocks.append(b)
        self.qk_norm = any(b.qn_w is not None for b in self.blocks)
        self.drop_plan = None  # stochastic depth (set per step by set_drop_plan)
        # grouped weight-gradient launches write dW = ... instead of dW += ... while this is set: valid only where the caller has zeroed the
        # gradients and runs this stack's backward ONCE before it reads them (VTPTrainer's step sets it; the autograd boundary, which
        # must accumulate like nn.Parameter.grad does, never does).  Saves the 256-KiB read of every output tile in the epilogue of the
        # step's dominant kernel: 38 -> 24 us per last-arriving workgroup (tools/wgrad_timeline.py)
        self.wgrad_overwrite = False  # (nothing enforces the single backward while it is set: ADVICE; a pull request of its own)
        self.wgrad_scratch: Dict[str, torch.Tensor] = {}  # partial sums / tickets shared by this stack's grouped launches
        # packed captions (TextEngine, causal + arg-max pooling): a RowPlan on the device.  Launch geometry stays that of the static
        # M = B * T; the kernels read the counts (ops: m_rows / k_rows / the varlen attention).  Set by the owner before forward() and left
        # in place for the matching backward(); None: padded rows.
        self.varlen: Optional[RowPlan] = None

    @property
    def m_rows(self):
        """device row limit of every row-wise launch: the live-row count of the packed captions, None for padded rows"""
        return None if self.varlen is None else self.varlen.rows

    def _rope_plan(self, ws: Workspace, segs, prefix_tokens: int, M: int):
        """(rope_pos int32 [M], sin, cos) for the fused qkv + RoPE epilogue: rope_pos[m] = row of the concatenated per-segment
        tables that rotates token row m, -1 for prefix (cls) rows.  Built once per workspace (static segment structure).  Under
        train-time RoPE augmentation the segments carry RopeAugTabs: sin / cos are then the static per-block buffers [depth, P, 64]
        themselves (refreshed in place every step; block i uses [i]), not a concatenated copy."""
        if self.style != "vit" or all(rp is None for _, _, rp in segs) or (2 * self.D) % 128 or self.qk_norm:
            return None  # (with QK normalisation the rotation follows the norm: it cannot ride in the projection's epilogue)
        hit = getattr(ws, "_rope_plan", None)
        aug = [rp for _, _, rp in segs if isinstance(rp, RopeAugTabs)]
        key = tuple((b, n, None if rp is None else (rp.sin_all.data_ptr(), rp.off) if isinstance(rp, RopeAugTabs) else rp[0].data_ptr())
                    for b, n, rp in segs) + (prefix_tokens,)
        if hit is not None and hit[0] == key:
            return hit[1]
        pos, tabs_s, tabs_c, base = [], [], [], 0
        for Bs, Ns, rp in segs:
            if rp is None:
                pos.append(torch.full((Bs * Ns,), -1, dtype=torch.int32))
                continue
            hw = _rope_hw(rp)
            assert Ns - prefix_tokens == hw, (Ns, prefix_tokens, hw)
            if aug:  # rows of the shared per-block buffers: the item's offset there
                assert isinstance(rp, RopeAugTabs) and rp.sin_all is aug[0].sin_all, "augmented and plain RoPE tables cannot be mixed in one pass"
                base = rp.off
            one = torch.cat([torch.full((prefix_tokens,), -1, dtype=torch.int32), torch.arange(hw, dtype=torch.int32) + base])
            pos.append(one.repeat(Bs))
            if not aug:
                tabs_s.append(rp[0])
                tabs_c.append(rp[1])
                base += hw
        dev = self.store.device
        if aug:
            plan = (torch.cat(pos).to(dev), aug[0].sin_all, aug[0].cos_all)
        else:
            plan = (torch.cat(pos).to(dev), torch.cat(tabs_s).contiguous(), torch.cat(tabs_c).contiguous())
        assert plan[0].numel() == M
        ws._rope_plan = (key, plan)
        return plan

    @staticmethod
    def _plan_tabs(plan, i: int):
        """sin / cos operands of the fused epilogue for block i"""
        if plan[1].ndim == 3:  # static per-block buffers of RopeAugTabs (refreshed in place); [1, P, 64]: one draw for every block
            i = min(i, plan[1].shape[0] - 1)
            return plan[1][i], plan[2][i]
        return plan[1], plan[2]

    # ------------------------------------------------------------------------------------------------ stochastic depth
    # block.py:20-118 (get_branges_scales) and :207-289: in training with drop_ratio > 0 every residual branch of every block runs
    # on a fresh random subset of the images of each list item and is added back with alpha = batch / kept.
    @staticmethod
    def drop_allocation(b: int, ratio: float, world: int = 1, rank: int = 0):
        """(images kept on this rank, residual scale factor) -- the reference's allocation rule: without DDP keep =
        max(int(b (1 - r)), 1), scale = b / keep; with DDP the GLOBAL keep count max(int(b W (1 - r)), W) is spread evenly over the
        ranks and scale = global batch / global kept (block.py:44-62; deterministic, so no broadcast is needed here)."""
        if world <= 1:
            keep = max(int(b * (1 - ratio)), 1)
            return keep, b / keep
        gb = b * world
        gkeep = max(int(gb * (1 - ratio)), world)
        base, extra = gkeep // world, gkeep % world
        alloc = [min(base + (1 if i < extra else 0), b) for i in range(world)]
        return alloc[rank], gb / max(sum(alloc), 1)

    def make_drop_plan(self, segs, ratio, generator: Optional[torch.Generator] = None, world: int = 1, rank: int = 0):
        """Host side, once per step: a random image subset per (block, branch, list item).  `ratio`: one rate, or one per list item
        (the reference has a rate per objective -- clip_drop_rate / ssl_drop_rate / rec_drop_rate, vtp.py:205-207 -- and the
        objectives are items of one list forward here).  Returns a dict with the int32 index tensor (CPU; copy it into the static
        device buffer with set_drop_plan) and the static shape information."""
        ratios = list(ratio) if isinstance(ratio, (list, tuple)) else [ratio] * len(segs)
        assert len(ratios) == len(segs)
        keeps, scales = [], []
        for (B, _, _), r in zip(segs, ratios):
            k, sc = self.drop_allocation(B, r, world, rank)
            keeps.append(k)
            scales.append(sc)
        per = sum(keeps)
        idx = torch.empty(self.depth * 2 * per, dtype=torch.int32)
        o = 0
        for _ in range(self.depth * 2):
            for (B, _, _), k in zip(segs, keeps):
                idx[o:o + k] = torch.randperm(B, generator=generator)[:k].to(torch.int32)
                o += k
        return dict(idx=idx, keeps=keeps, scales=scales, per=per, ratio=ratio, batches=[B for B, _, _ in segs])

    def set_drop_plan(self, plan, ws_key="drop"):
        """activate / update (plan) or switch off (None) stochastic depth for the following forward + backward.  The device index
        buffer of a given size is allocated ONCE and kept for the lifetime of the stack: captured hipGraph segments bake its
        address, so it is only ever refreshed in place -- switching the plan off, or alternating between plans of different sizes
        (steps with / without SSL crops), never frees or moves a buffer a graph may still read."""
        if plan is not None and self.style != "vit":
            raise NotImplementedError("stochastic depth is a property of the ViT blocks (block.py:207-289); the text tower has none")
        if plan is None:
            if self.drop_plan is not None:
                self.last_drop_plan = self.drop_plan  # introspection (tests replay the subsets of the step that just ran)
            self.drop_plan = None
            return
        bufs = self.__dict__.setdefault("_drop_bufs", {})
        n = plan["idx"].numel()
        buf = bufs.get(n)
        if buf is None:
            buf = bufs[n] = torch.empty(n, dtype=torch.int32, device=self.store.device)
        buf.copy_(plan["idx"], non_blocking=True)
        cur = dict(plan)
        cur["idx_dev"] = buf
        self.drop_plan = cur

    @staticmethod
    def _check_drop_plan(p, segs):
        """the plan was drawn for specific per-item batch sizes: a pass with other shapes must not run on it (out-of-range image
        indices / silently truncated item lists)"""
        got = [B for B, _, _ in segs]
        if p.get("batches") != got:
            raise RuntimeError(f"stochastic-depth plan drawn for item batch sizes {p.get('batches')} used on a pass with {got}")

    def _drop_idx(self, i: int, branch: int, s: int):
        p = self.drop_plan
        o = (i * 2 + branch) * p["per"] + sum(p["keeps"][:s])
        return p["idx_dev"][o:o + p["keeps"][s]]

    def _drop_segs(self, segs):
        """(the compact list [(kept images, N_i, rope_i)], its row count) of the active plan for a pass over `segs`"""
        self._check_drop_plan(self.drop_plan, segs)
        csegs = [(k, N, rp) for (_, N, rp), k in zip(segs, self.drop_plan["keeps"])]
        return csegs, sum(k * N for k, N, _ in csegs)

    def _gather(self, x, segs, csegs, i, branch, dst, dst_b, scale_by_seg):
        D = self.D
        r_full, r_c = 0, 0
        for s, ((B, N, _), (k, _, _)) in enumerate(zip(segs, csegs)):
            sc = scale_by_seg[s] if isinstance(scale_by_seg, (list, tuple)) else scale_by_seg
            ops.gather_image_rows(x[r_full:], self._drop_idx(i, branch, s), None if dst is None else dst[r_c:],
                                  None if dst_b is None else dst_b[r_c:], k, N, D, sc)
            r_full += B * N
            r_c += k * N

    def _scatter(self, src, x, segs, csegs, i, branch, alpha_by_seg, accumulate):
        D = self.D
        r_full, r_c = 0, 0
        for s, ((B, N, _), (k, _, _)) in enumerate(zip(segs, csegs)):
            al = alpha_by_seg[s] if isinstance(alpha_by_seg, (list, tuple)) else alpha_by_seg
            ops.scatter_image_rows(src[r_c:], self._drop_idx(i, branch, s), x[r_full:], k, N, D, al, accumulate)
            r_full += B * N
            r_c += k * N

    @staticmethod
    def _rows(segs):
        """(first row, B, N, rope) of every segment of a row-concatenated token buffer."""
        r0 = 0
        for B, N, rope in segs:
            yield r0, B, N, rope
            r0 += B * N

    @staticmethod
    def _attn_rows(segs):
        """_rows with neighbouring segments of equal sequence length and the same RoPE tables merged into one batch (the clean
        images and the global crops of a list forward: one attention launch instead of two, a better last round of workgroups)."""
        out = []
        for r0, B, N, rope in Stack._rows(segs):
            same = out and (out[-1][3] is rope or (isinstance(out[-1][3], tuple) and isinstance(rope, tuple)
                                                   and out[-1][3][0] is rope[0] and out[-1][3][1] is rope[1]))
            if out and out[-1][2] == N and same:  # (RopeAugTabs of different items never merge: each item has its own draws)
                out[-1] = (out[-1][0], out[-1][1] + B, N, rope)
            else:
                out.append((r0, B, N, rope))
        return out

    # ------------------------------------------------------------------------------------------------ the two half-blocks
    # Every pass runs them over a branch input of M rows: the full residual in the plain pass (the output then adds back through the
    # fused resid= epilogue), the gathered rows of the kept images under stochastic depth (the output goes to `delta`, which the
    # caller scatters back with alpha).  `t` prefixes the workspace keys of what the branch keeps for the backward.
    def _attention(self, qkv, o, lse, rows, i: int, prefix_tokens: int, rope_qk: bool):
        """per-segment RoPE (unless the qkv projection applied it: rope_qk False) + attention over qkv [M, 3D] -> o [M, D]"""
        D, heads = self.D, self.heads
        if self.varlen is not None:
            (r0, Bs, Ns, rp), = rows
            assert rp is None and self.causal
            ops.attn_fwd_varlen(qkv, qkv[:, D:], qkv[:, 2 * D:], o, lse, self.varlen.cu, Bs, Ns, heads, 3 * D, D, ATTN_SCALE)
            return
        for r0, Bs, Ns, rp in rows:
            q_s, o_s = qkv[r0:r0 + Bs * Ns], o[r0:r0 + Bs * Ns]
            if rp is not None and rope_qk:
                rs, rc = rope_at(rp, i)
                ops.rope_qk(q_s, rs, rc, Bs, Ns, heads, prefix_tokens)
            ops.attn_fwd(q_s, q_s[:, D:], q_s[:, 2 * D:], o_s, lse[r0 * heads:], Bs, Ns, heads, Ns * 3 * D, 3 * D, Ns * D, D,
                         ATTN_SCALE, self.causal)

    def _attn_fwd(self, ws: Workspace, t: str, i: int, x, out, resid, M: int, rows, prefix_tokens: int, rope_plan, proj: bool = True):
        """out = (resid +) proj(attn(rope(qkv(norm1(x)))));  returns (xn1, st1, qkv, o, lse).  proj=False: stops behind the attention
        (the caller projects a subset of the rows of o)"""
        D, heads, b = self.D, self.heads, self.blocks[i]
        mr = self.m_rows
        xn1, st1 = ws.get(t + "xn1", (M, D), BF), ws.get(t + "st1", (M, 2), F32)
        qkv, o = ws.get(t + "qkv", (M, 3 * D), BF), ws.get(t + "o", (M, D), BF)
        lse = ws.get(t + "lse", (M * heads,), F32)  # per segment [B_i, heads, N_i]
        ops.norm_fwd(x, b.n1w, b.n1b, xn1, st1, M, D, self.eps, self.kind, m_rows=mr)
        if rope_plan is not None:  # apply_rope rides in the epilogue of the qkv projection (all segments, one launch)
            ps, pc = self._plan_tabs(rope_plan, i)
            ops.gemm_qkv_rope(xn1, b.qkv.w, b.qkv.bias, qkv, M, 3 * D, D, rope_plan[0], ps, pc, 2 * D)
        elif b.qn_w is not None:  # projection -> QK norm (attention.py:67-68,119-120; pre-norm values and 1/rms kept) -> RoPE below
            qkv_pre = ws.get(t + "qkv_pre", (M, 3 * D), BF)
            qinv = ws.get(t + "qinv", (M, 2 * heads), F32)
            ops.gemm_nt(xn1, b.qkv.w, qkv_pre, M=M, N=3 * D, K=D, bias=b.qkv.bias, epi=EPI_BF16)
            ops.qk_norm_fwd(qkv_pre, b.qn_w, b.kn_w, qkv, qinv, M, D)
        else:
            ops.gemm_nt(xn1, b.qkv.w, qkv, M=M, N=3 * D, K=D, bias=b.qkv.bias, epi=EPI_BF16, m_rows=mr)
        self._attention(qkv, o, lse, rows, i, prefix_tokens, rope_plan is None)
        if proj:
            ops.gemm_nt(o, b.proj.w, out, M=M, N=D, K=D, bias=b.proj.bias, gamma=b.ls1, resid=resid, epi=EPI_F32, m_rows=mr)
        return xn1, st1, qkv, o, lse

    def _ffn_fwd(self, ws: Workspace, t: str, i: int, x, out, resid, M: int, train: bool):
        """out = (resid +) w3(act(w12 / fc(norm2(x))));  returns (xn2, st2, pre, hid) -- pre (the FFN pre-activations) only in training"""
        D, H, b = self.D, self.H, self.blocks[i]
        mr = self.m_rows
        xn2, st2 = ws.get(t + "xn2", (M, D), BF), ws.get(t + "st2", (M, 2), F32)
        pre = ws.get(t + "x12", (M, 2 * H if self.swiglu else H), BF) if train else None
        hid = ws.get(t + "hid", (M, H), BF)
        ops.norm_fwd(x, b.n2w, b.n2b, xn2, st2, M, D, self.eps, self.kind, m_rows=mr)
        if self.swiglu:
            ops.gemm_nt(xn2, b.w12.w12, hid, M=M, N=2 * H, K=D, c2=pre, ldc2=2 * H, bias=b.w12.b12, epi=EPI_SWIGLU, m_rows=mr)
        else:  # Mlp FFN (ffn_layer = "mlp", ffn.py:21-48; the text tower's c_fc / c_proj): fc1 -> GELU -> fc2
            ops.gemm_nt(xn2, b.fc.w, hid, M=M, N=H, K=D, c2=pre, ldc2=H, bias=b.fc.bias,
                        epi=ops.EPI_QUICK_GELU if self.quick_gelu else EPI_GELU, m_rows=mr)
        ops.gemm_nt(hid, b.w3.w, out, M=M, N=D, K=H, bias=b.w3.bias, gamma=b.ls2, resid=resid, epi=EPI_F32, m_rows=mr)
        return xn2, st2, pre, hid

    def _ffn_bwd(self, ws: Workspace, i: int, s: BlockSaved, dy, dy_b, dx, dx_b, M: int, bt: str, dpre, *, fused: bool,
                 bias_done: bool = False, probs=None, dx_colsum=None):
        """dy / dy_b: gradient of the FFN branch output (f32 / bf16 copy); dx (+ dx_b) = dy + the gradient through the branch into its
        input.  fused: the SwiGLU backward rides in the w3 dgrad's epilogue.  probs: collects the grouped weight-gradient problems."""
        D, H, b = self.D, self.H, self.blocks[i]
        mr = self.m_rows
        dh, dxn = ws.get(bt + "dh", (M, H), BF), ws.get(bt + "dxn", (M, D), BF)
        linear_bwd(ws, "w3", b.w3, dy_b, s.hid, M, dpre if fused else dh, bias_grad_done=bias_done,
                   ls=(b.ls2, b.gls2) if b.ls2 is not None else None, dgrad_swiglu=s.pre if fused else None, defer=probs, m_rows=mr)
        OVERLAP.run_deferred()  # side work forked at the block boundary: behind the block's first main-stream kernel
        if self.swiglu:
            if not fused:
                ops.swiglu_bwd(dh, s.pre, dpre, M, H)
            linear_bwd(ws, "w12", None, dpre, s.xn2, M, dxn, N=2 * H, K=D, gw=b.w12.gw1, gb=b.w12.gb1, wT=b.w12.w12T, swiglu_h=H,
                       defer=probs)
        else:
            ops.gelu_bwd(dh, s.pre, dpre, M * H, quick=self.quick_gelu, m_rows=mr, H=H)
            linear_bwd(ws, "fc", b.fc, dpre, s.xn2, M, dxn, defer=probs, m_rows=mr)
        ops.norm_bwd(dxn, s.ffn_in, b.n2w, s.st2, dy, dx, dx_b, b.gn2w, b.gn2b, M, D, self.kind, dx_colsum=dx_colsum, m_rows=mr)

    def _attn_bwd(self, ws: Workspace, t: str, i: int, s: BlockSaved, dy, dy_b, dx, dx_b, M: int, bt: str, dqkv, rows,
                  prefix_tokens: int, *, bias_done: bool = False, probs=None, join: bool = False, dx_colsum=None):
        """_ffn_bwd of the attention branch.  join: wait for the side stream before norm1's backward (which overwrites the dy
        operand of the previous block's grouped weight gradients).  With tail rows (s.row_map set) dy / dy_b are the COMPACT [Mc, D]
        gradients: the projection's dgrad and weight gradient run on them, d_o is expanded to all M rows for the attention backward
        (every row is a key / value), and norm1's backward picks its residual gradient through the row map."""
        D, heads, b = self.D, self.heads, self.blocks[i]
        mr = self.m_rows
        d_o, dxn = ws.get(bt + "do", (M, D), BF), ws.get(bt + "dxn", (M, D), BF)
        delta = ws.get(bt + "delta", (M * heads,), F32)
        if s.row_map is not None:
            Mc = s.o_c.shape[0]
            d_o_c = ws.get(bt + "do", (Mc, D), BF)
            linear_bwd(ws, "proj", b.proj, dy_b, s.o_c, Mc, d_o_c, bias_grad_done=bias_done, defer=probs)
            ops.expand_rows_bf16(d_o_c, s.row_map, d_o, M, Mc, D)
        else:
            linear_bwd(ws, "proj", b.proj, dy_b, s.o, M, d_o, bias_grad_done=bias_done,
                       ls=(b.ls1, b.gls1) if b.ls1 is not None else None, defer=probs, m_rows=mr)
        if self.varlen is not None:
            (r0, Bs, Ns, rp), = rows
            ops.attn_bwd_varlen(s.qkv, s.qkv[:, D:], s.qkv[:, 2 * D:], s.o, d_o, s.lse, delta, dqkv, dqkv[:, D:], dqkv[:, 2 * D:],
                                self.varlen.cu, Bs, Ns, heads, 3 * D, D, ATTN_SCALE)
            rows = ()
        for r0, Bs, Ns, rp in rows:
            r1 = r0 + Bs * Ns
            q_s, dq_s = s.qkv[r0:r1], dqkv[r0:r1]
            # dq / dk come back as gradients w.r.t. the un-rotated q, k (inverse RoPE fused into the attention backward)
            ops.attn_bwd(q_s, q_s[:, D:], q_s[:, 2 * D:], s.o[r0:r1], d_o[r0:r1], s.lse[r0 * heads:], delta[r0 * heads:], dq_s,
                         dq_s[:, D:], dq_s[:, 2 * D:], Bs, Ns, heads, Ns * 3 * D, 3 * D, Ns * D, D, ATTN_SCALE, self.causal,
                         rope=None if rp is None else rope_at(rp, i), rope_prefix=prefix_tokens)
        if b.qn_w is not None:  # gradient w.r.t. the normalised q, k -> w.r.t. the projection output (in place), + dw
            ops.qk_norm_bwd(dqkv, ws.get(t + "qkv_pre", (M, 3 * D), BF), ws.get(t + "qinv", (M, 2 * heads), F32), b.qn_w, b.kn_w,
                            b.g_qn, b.g_kn, M, D)
        linear_bwd(ws, "qkv", b.qkv, dqkv, s.xn1, M, dxn, defer=probs, m_rows=mr)
        if join:
            OVERLAP.join()
        if s.row_map is not None:
            ops.norm_bwd_rows(dxn, s.attn_in, b.n1w, s.st1, dy, s.row_map, dx, dx_b, b.gn1w, b.gn1b, M, D, self.kind, dx_colsum=dx_colsum)
        else:
            ops.norm_bwd(dxn, s.attn_in, b.n1w, s.st1, dy, dx, dx_b, b.gn1w, b.gn1b, M, D, self.kind, dx_colsum=dx_colsum, m_rows=mr)

    def varlen_ok(self, M: int) -> bool:
        """may a pass over M static token rows run on packed captions (self.varlen)?  Causal blocks without RoPE, QK norm, LayerScale,
        stochastic depth or the fp8 forward, and a token count at which the backward takes the grouped weight gradients (the only
        weight-gradient path that reads the row count)"""
        D, H = self.D, self.H
        return (self.causal and not self.qk_norm and self.drop_plan is None and getattr(self, "fp8", None) is None
                and all(b.ls1 is None and b.ls2 is None for b in self.blocks) and M >= 256 and D % 8 == 0 and H % 8 == 0
                and ops.wgrad_group_fits(M, max(3 * D, 2 * H if self.swiglu else H)))

    # x: f32 [M, D] input residual.  Returns the output residual (f32 [M, D]).
    def tail_rows_ok(self, train: bool) -> bool:
        """may forward() take a tail row plan?  Not under stochastic depth (the branches already run on gathered rows), not on the fp8
        forward or its calibration pass, not with LayerScale; VTP_TAIL_ROWS=0 keeps the full path (same-box A/B runs)"""
        return (_env_flag("VTP_TAIL_ROWS") and self.style == "vit" and not (train and self.drop_plan is not None)
                and getattr(self, "fp8", None) is None and self.D % 8 == 0 and self.D <= 1024
                and self.blocks[-1].ls1 is None and self.blocks[-1].ls2 is None)

    def forward(self, ws: Workspace, x, segs, prefix_tokens: int, train: bool, tail=None, fp32: bool = False, keep: bool = False):
        """`segs` = [(B_i, N_i, rope_i)]: several batches of different sequence length concatenated along the token-row
        axis (the reference's list path, block.py:235-298 / utils.py:14-25 cat_keep_shapes): every linear / norm runs once
        over all rows, RoPE and attention run per segment on its row range.  In training with a drop plan set (stochastic depth)
        `x` is updated IN PLACE block after block and each branch runs on the gathered rows of its kept images.
        tail = (idx int32 [T] on the device, T, L): only rows [0, L) and L + idx[t] of the output are read (idx[t] = -1: padding).  The
        LAST block then runs everything behind its attention -- proj, norm2, the FFN: all row-wise -- on those Mc = L + T rows alone
        (its attention still sees every row: all of them are keys and values) and the output has Mc rows: [0, L) unchanged, L + t =
        full row L + idx[t], zero-input rows for the padding.  The kept rows are bit-identical to the full pass."""
        D = self.D
        M = sum(b * n for b, n, _ in segs)
        if fp32:  # the fp32 inference forward (_forward_fp32): plain full rows, inference only
            if train or tail is not None or self.varlen is not None:
                raise RuntimeError("Stack.forward: the fp32 forward is an inference pass over plain full rows (no train, tail or packed rows)")
            return self._forward_fp32(ws, x, segs, prefix_tokens, M, keep)
        if tail is not None and not self.tail_rows_ok(train):
            raise RuntimeError("Stack.forward: a tail row plan was passed to a pass that cannot take one (tail_rows_ok)")
        if self.varlen is not None and not (self.varlen_ok(M) and tail is None and len(segs) == 1 and segs[0][2] is None):
            raise RuntimeError("Stack.forward: packed captions were set on a pass that cannot take them (varlen_ok, one segment, no RoPE)")
        fp8 = getattr(self, "fp8", None)
        if fp8 is not None and fp8["ready"] and not train:
            return self._forward_fp8(ws, x, segs, prefix_tokens, M)
        calib = fp8["amax"] if (fp8 is not None and not fp8["ready"] and not train) else None
        drop = train and self.drop_plan is not None
        if drop:
            csegs, Mb = self._drop_segs(segs)
            rows, scales = list(self._rows(csegs)), self.drop_plan["scales"]
        else:
            csegs, Mb, rows = segs, M, self._attn_rows(segs)
        rope_plan = self._rope_plan(ws, csegs, prefix_tokens, Mb)
        saved_all = []
        for i in range(self.depth):
            if drop:
                t = f"{i}.d."
                x1, x2 = ws.get(t + "xs1", (Mb, D), F32), ws.get(t + "xs2", (Mb, D), F32)
                delta = ws.get("d.delta", (Mb, D), F32)
                self._gather(x, segs, csegs, i, 0, x1, None, 1.0)
                a = self._attn_fwd(ws, t, i, x1, delta, None, Mb, rows, prefix_tokens, rope_plan)
                self._scatter(delta, x, segs, csegs, i, 0, scales, accumulate=True)  # x_attn = index_add(x, residual, alpha)
                self._gather(x, segs, csegs, i, 1, x2, None, 1.0)  # the FFN branch on an independent subset
                f = self._ffn_fwd(ws, t, i, x2, delta, None, Mb, True)
                self._scatter(delta, x, segs, csegs, i, 1, scales, accumulate=True)
            else:
                t = f"{i}." if train else ""
                tl = tail if i == self.depth - 1 else None
                Mo = M if tl is None else tl[2] + tl[1]  # rows behind the attention
                x1, x2 = x, ws.get(t + "xmid", (Mo, D), F32)  # the block input (previous block's xout) is kept for norm1 backward
                xout = ws.get((f"{i}.xout" if train else f"xout{i & 1}"), (Mo, D), F32)
                a = self._attn_fwd(ws, t, i, x1, x2, x1, M, rows, prefix_tokens, rope_plan, proj=tl is None)
                if tl is not None:
                    idx, T, L = tl
                    o_c, x_c = ws.get(t + "o_c", (Mo, D), BF), ws.get(t + "x_c", (Mo, D), F32)
                    ops.gather_tail_rows(a[3], x1, idx, o_c, x_c, T, L, M, D)
                    b = self.blocks[i]
                    ops.gemm_nt(o_c, b.proj.w, x2, M=Mo, N=D, K=D, bias=b.proj.bias, resid=x_c, epi=EPI_F32)
                    if train:
                        row_map = ws.get(t + "row_map", (M,), torch.int32)
                        ops.tail_row_map(idx, row_map, T, L, M)
                        extra_saved = (o_c, row_map)
                f = self._ffn_fwd(ws, t, i, x2, xout, x2, Mo, train)
                if calib is not None:  # fp8 calibration pass: amax of the four GEMM inputs of this block
                    for j, tns in enumerate((a[0], a[3], f[0], f[3])):
                        ops.amax(tns, calib[i, j:j + 1])
                x = xout
            if train:
                saved_all.append(BlockSaved(x1, *a, x2, *f, *(extra_saved if (not drop and tl is not None) else ())))
        self.last_saved = saved_all  # per-call context: several forward passes may be in flight before their backward
        return x

    # ---- fp8 (e4m3) inference forward: BASELINE config 5 (per-tensor scales: weights from their own amax, activations from a
    # calibration pass of the bf16 path over representative images)
    def fp8_begin_calibration(self):
        if not self.swiglu or self.D % 16 or self.H % 16 or any(b.ls1 is not None or b.ls2 is not None for b in self.blocks):
            raise NotImplementedError("fp8 forward: SwiGLU ViT blocks with D, H multiples of 16, no LayerScale")
        dev = self.store.device
        self.fp8 = {"ready": False, "amax": torch.zeros(self.depth, 4, dtype=F32, device=dev)}

    def fp8_finalize(self):
        """weights -> e4m3 with scale 448 / amax(W); activation scales 448 / calibrated amax (x 1 / margin)"""
        f, dev = self.fp8, self.store.device
        bad = (~torch.isfinite(f["amax"])).nonzero().cpu().tolist()  # a NaN / inf that arose in the calibration pass (vtp_amax keeps it)
        if bad:
            raise ValueError(f"fp8 calibration: the amax of block {bad[0][0]}, operand {bad[0][1]} (0 qkv, 1 proj, 2 w12, 3 w3 input) is "
                             f"not finite ({float(f['amax'][bad[0][0], bad[0][1]])}): the calibration batch produced a NaN or an overflow")
        amax = f["amax"].clamp_min(1e-12)
        f["act_scale"] = (ops.E4M3_MAX / amax).contiguous()        # device [depth, 4]: read by the quantise kernels
        act_inv = (amax / ops.E4M3_MAX).cpu().tolist()               # host: the GEMM alphas
        f["w"], f["alpha"] = [], []
        for i, b in enumerate(self.blocks):
            ws8, al = [], []
            for j, w in enumerate((b.qkv.w, b.proj.w, b.w12.w12, b.w3.w)):
                wa = float(w.float().abs().max().clamp_min(1e-12))
                q = torch.empty(w.shape, dtype=torch.uint8, device=dev)
                ops.quantize_e4m3(w.contiguous(), q, ops.E4M3_MAX / wa)
                ws8.append(q)
                al.append(act_inv[i][j] * wa / ops.E4M3_MAX)
            f["w"].append(ws8)
            f["alpha"].append(al)
        f["ready"] = True

    def _forward_fp8(self, ws: Workspace, x, segs, prefix_tokens: int, M: int):
        """Stack.forward(train=False) with the four linear maps of every block on the fp8 MFMA path: norm / attention / SwiGLU
        outputs are quantised (one extra row pass each) and multiplied against e4m3 weights; accumulation, bias, residual and
        the attention itself are unchanged (fp32 / bf16)."""
        D, H, heads, f = self.D, self.H, self.heads, self.fp8
        a8 = ws.get("f8.a", (M, max(D, H)), torch.uint8)
        qkv = ws.get("qkv", (M, 3 * D), BF)
        o = ws.get("o", (M, D), BF)
        lse = ws.get("lse", (M * heads,), F32)
        xmid = ws.get("xmid", (M, D), F32)
        hid = ws.get("hid", (M, H), BF)
        rope_plan = self._rope_plan(ws, segs, prefix_tokens, M)
        rope_arg = None if rope_plan is None else (rope_plan[0], rope_plan[1], rope_plan[2], 2 * D)
        rows = self._attn_rows(segs)
        for i, b in enumerate(self.blocks):
            w8, al, sc = f["w"][i], f["alpha"][i], f["act_scale"][i]
            xout = ws.get(f"xout{i & 1}", (M, D), F32)
            ops.norm_fwd_e4m3(x, b.n1w, b.n1b, a8, sc[0:1], None, M, D, self.eps, self.kind)  # norm + quantise in one pass
            if b.qn_w is not None:  # QK normalisation: e4m3 projection -> bf16 pre-norm q, k -> RMSNorm(head_dim) -> RoPE below
                qkv_pre = ws.get("f8.qkv_pre", (M, 3 * D), BF)
                ops.gemm_nt_fp8(a8, w8[0], qkv_pre, M=M, N=3 * D, K=D, alpha=al[0], bias=b.qkv.bias, epi=EPI_BF16)
                ops.qk_norm_fwd(qkv_pre, b.qn_w, b.kn_w, qkv, ws.get("f8.qinv", (M, 2 * heads), F32), M, D)
            else:
                ops.gemm_nt_fp8(a8, w8[0], qkv, M=M, N=3 * D, K=D, alpha=al[0], bias=b.qkv.bias, epi=EPI_BF16, rope=rope_arg)
            self._attention(qkv, o, lse, rows, i, prefix_tokens, rope_arg is None)
            ops.quantize_e4m3(o, a8, sc[1:2])
            ops.gemm_nt_fp8(a8, w8[1], xmid, M=M, N=D, K=D, alpha=al[1], bias=b.proj.bias, resid=x, epi=EPI_F32)
            ops.norm_fwd_e4m3(xmid, b.n2w, b.n2b, a8, sc[2:3], None, M, D, self.eps, self.kind)
            ops.gemm_nt_fp8(a8, w8[2], hid, M=M, N=2 * H, K=D, alpha=al[2], bias=b.w12.b12, epi=EPI_SWIGLU)
            ops.quantize_e4m3(hid, a8, sc[3:4])
            ops.gemm_nt_fp8(a8, w8[3], xout, M=M, N=D, K=H, alpha=al[3], bias=b.w3.bias, resid=xmid, epi=EPI_F32)
            x = xout
        return x

    # ---- fp32 inference forward: the reference with fp32 weights and no autocast (oracle/vtp_oracle.py on fp32 tensors)
    def fp32_check(self, what: str):
        """the configurations the fp32 forward does not cover raise here -- before any launch, never a silent bf16 pass"""
        if self.qk_norm:
            raise NotImplementedError(f"fp32 forward ({what}): QK normalisation (use_qk_norm) is not implemented in fp32")
        if self.D % 8 or self.H % 8 or self.D != self.heads * 64:
            raise NotImplementedError(f"fp32 forward ({what}): needs D, H multiples of 8 and head dimension 64 (D={self.D} H={self.H} heads={self.heads})")

    def _forward_fp32(self, ws: Workspace, x, segs, prefix_tokens: int, M: int, keep: bool = False):
        """Stack.forward(train=False) in fp32 throughout: norms, the four linear maps (operands = the fp32 master parameters, products on
        the f32-input MFMA, one fmaf chain per output element), attention with an fp32 online softmax, activations and residuals.
        apply_rope keeps the reference's cast of q and k to the RoPE dtype (attention.py:70-89).  Plain full rows: no tail-row plan, no
        packed captions, no stochastic depth.  keep: every block's output stays in its own buffer "f32.{i}.xout"."""
        self.fp32_check(self.style)
        D, H, heads = self.D, self.H, self.heads
        xn, st = ws.get("f32.xn", (M, D), F32), ws.get("f32.st", (M, 2), F32)
        qkv, o = ws.get("f32.qkv", (M, 3 * D), F32), ws.get("f32.o", (M, D), F32)
        xmid, hid = ws.get("f32.xmid", (M, D), F32), ws.get("f32.hid", (M, H), F32)
        rows = self._attn_rows(segs)
        for i, b in enumerate(self.blocks):
            xout = ws.get(f"f32.{i}.xout" if keep else f"f32.xout{i & 1}", (M, D), F32)
            ops.norm_fwd_f32(x, b.n1w, b.n1b, xn, st, M, D, self.eps, self.kind)
            ops.gemm_nt_f32(xn, b.qkv.w32, qkv, M=M, N=3 * D, K=D, bias=b.qkv.bias)
            for r0, Bs, Ns, rp in rows:
                q_s, o_s = qkv[r0:r0 + Bs * Ns], o[r0:r0 + Bs * Ns]
                if rp is not None:
                    rs, rc = rope_at(rp, i)
                    ops.rope_qk_f32(q_s, rs, rc, Bs, Ns, heads, prefix_tokens)
                ops.attn_fwd_f32(q_s, q_s[:, D:], q_s[:, 2 * D:], o_s, Bs, Ns, heads, Ns * 3 * D, 3 * D, Ns * D, D, ATTN_SCALE, self.causal)
            ops.gemm_nt_f32(o, b.proj.w32, xmid, M=M, N=D, K=D, bias=b.proj.bias, gamma=b.ls1, resid=x, epi=ops.F32_RESID)
            ops.norm_fwd_f32(xmid, b.n2w, b.n2b, xn, st, M, D, self.eps, self.kind)
            if self.swiglu:
                ops.gemm_nt_f32(xn, b.w1_32, hid, M=M, N=H, K=D, w2=b.w2_32, bias=b.b1_32, bias2=b.b2_32, epi=ops.F32_SWIGLU)
            else:
                ops.gemm_nt_f32(xn, b.fc.w32, hid, M=M, N=H, K=D, bias=b.fc.bias,
                                epi=ops.F32_QUICK_GELU if self.quick_gelu else ops.F32_GELU)
            ops.gemm_nt_f32(hid, b.w3.w32, xout, M=M, N=D, K=H, bias=b.w3.bias, gamma=b.ls2, resid=xmid, epi=ops.F32_RESID)
            x = xout
        return x

    def w3_colsum_target(self, i: int):
        """where the norm backward in front of block i's w3 gradient may add the column sums of its bf16 output (= w3's bias
        gradient); None when a LayerScale sits between them (the bias gradient then needs the gamma factor) or under
        stochastic depth (the FFN branch sees a gathered subset of the rows)"""
        b = self.blocks[i]
        return b.w3.gb if (b.ls2 is None and self.drop_plan is None) else None

    # dy: f32 [M,D] grad of the stack output, dy_b: its bf16 copy.  Returns (dx f32, dx bf16) for the stack input.
    def backward(self, ws: Workspace, dy, dy_b, segs, prefix_tokens: int, saved=None, dy_colsum_done: bool = False,
                 hold_last: bool = False, extra_last=None):
        """Generator: yields ("block", i) each time all parameter gradients of block i have been enqueued (a gradient-bucket /
        graph-segment boundary for the trainer); returns (dx f32, dx bf16) of the stack input.  With a drop plan set (the forward
        ran with stochastic depth) `dy` is updated IN PLACE into that gradient and dy_b receives its bf16 copy.
        dy_colsum_done: the caller's norm backward already summed dy_b's columns into the last block's w3 bias gradient
        (self.blocks[-1].w3.gb as its dx_colsum).
        hold_last (grouped weight gradients only): block 0's group is neither launched nor announced here but left in self.held =
        (0, group) -- the caller launches it and yields ("block", 0) -- and extra_last, a list of wgrad.Problem records (dy and Ktok
        unset) over the same token rows whose dy is this stack's input gradient (TrunkEngine: the patch-embed weight gradient),
        rides in that launch.
        Tail rows (the forward ran with a row plan: saved[-1].row_map is set): dy / dy_b have the Mc compact rows, and the last block's
        FFN half, its projection and their weight gradients (K = Mc token rows) run on them -- see _attn_bwd."""
        D, H = self.D, self.H
        M = sum(b * n for b, n, _ in segs)
        saved = self.last_saved if saved is None else saved
        tail_Mc = saved[-1].o_c.shape[0] if saved and saved[-1].row_map is not None else None
        drop = self.drop_plan is not None
        if drop:
            csegs, Mb = self._drop_segs(segs)
            rows, scales, bt = list(self._rows(csegs)), self.drop_plan["scales"], "b.d."
            gdy, gdy_b = ws.get(bt + "gdy", (Mb, D), F32), ws.get(bt + "gdy_b", (Mb, D), BF)
            dxc = ws.get(bt + "dxc", (Mb, D), F32)
        else:
            Mb, rows, bt = M, self._attn_rows(segs), "b."
            dmid = ws.get("b.dmid", (M, D), F32)
        # grouped weight gradients: the four dW of block i are ONE launch (split-K combine and bias-gradient column sums inside
        # it), issued at the start of block i - 1's backward so that it overlaps that block's dgrad / attention kernels; the dy
        # operands it reads (dpre, dmid_b, dqkv; dy_b already alternates) are therefore double-buffered by block parity.  LayerScale,
        # stochastic depth and small token counts take the per-layer launches (ring-kernel fallback inside).
        grouped = not drop and M >= 256 and all(b.ls1 is None and b.ls2 is None for b in self.blocks) \
            and ops.wgrad_group_fits(M, max(3 * D, 2 * H if self.swiglu else H)) and D % 8 == 0 and H % 8 == 0
        vl = self.varlen
        if vl is not None and not (grouped and tail_Mc is None and len(segs) == 1 and not extra_last):
            raise RuntimeError("Stack.backward: packed captions need the grouped weight gradients of one plain segment (varlen_ok)")
        par = (lambda i: f".{i & 1}") if grouped else (lambda i: "")
        pending = None  # (block index, the block's planned launch: wgrad.plan_block) whose launch is due

        def launch_pending():
            """fork now (the side stream picks up behind the norm backward that closed the previous block); the launch itself is
            issued behind this block's first main-stream kernel (Overlap.defer)"""
            if pending is None:
                return
            if OVERLAP.enabled:
                OVERLAP.fork()
                side, grp = OVERLAP.side, pending[1]

                def issue():
                    with torch.cuda.stream(side):
                        grp.launch()
                OVERLAP.defer(issue)
            else:
                pending[1].launch()

        for i in range(self.depth - 1, -1, -1):
            b, s = self.blocks[i], saved[i]
            t = f"{i}.d." if drop else f"{i}."
            dpre = ws.get(bt + "dx12" + par(i), (Mb, 2 * H if self.swiglu else H), BF)
            dqkv = ws.get(bt + "dqkv" + par(i), (Mb, 3 * D), BF)
            if drop:
                # each branch: d(delta) = alpha * dy[kept rows]; the branch-input gradient lands on the same rows
                self._gather(dy, segs, csegs, i, 1, gdy, gdy_b, scales)
                self._ffn_bwd(ws, i, s, gdy, gdy_b, dxc, None, Mb, bt, dpre, fused=False)
                self._scatter(dxc, dy, segs, csegs, i, 1, 1.0, accumulate=False)
                self._gather(dy, segs, csegs, i, 0, gdy, gdy_b, scales)
                self._attn_bwd(ws, t, i, s, gdy, gdy_b, dxc, None, Mb, bt, dqkv, rows, prefix_tokens)
                self._scatter(dxc, dy, segs, csegs, i, 0, 1.0, accumulate=False)
                OVERLAP.join()
                yield ("block", i)
                continue
            dxo = ws.get(f"b.dx{i & 1}", (M, D), F32)
            dxo_b = ws.get(f"b.dx_b{i & 1}", (M, D), BF)
            Mf = tail_Mc if (tail_Mc is not None and i == self.depth - 1) else M  # rows of the block's FFN half
            if Mf != M:
                dpre = ws.get(bt + "dx12" + par(i), (Mf, 2 * H if self.swiglu else H), BF)
            dmid = ws.get("b.dmid", (Mf, D), F32)
            dmid_b = ws.get("b.dmid_b" + par(i), (Mf, D), BF)
            probs = [] if grouped else None
            if grouped:
                launch_pending()  # dW of block i + 1, beside this block's kernels
            # the norm backward kernels also sum the columns of their bf16 output = the bias gradient of the linear layer that
            # takes it as dy (proj after the FFN branch; the previous block's w3 after the attention branch)
            self._ffn_bwd(ws, i, s, dy, dy_b, dmid, dmid_b, Mf, bt, dpre, fused=self.swiglu and b.ls2 is None,
                          bias_done=dy_colsum_done if i == self.depth - 1 else self.w3_colsum_target(i) is not None, probs=probs,
                          dx_colsum=b.proj.gb if b.ls1 is None else None)
            # grouped: dW of block i + 1 is done before norm1's backward overwrites the dy operand it read (b.dx_b, same parity)
            self._attn_bwd(ws, t, i, s, dmid, dmid_b, dxo, dxo_b, M, bt, dqkv, rows, prefix_tokens, bias_done=b.proj.gb is not None,
                           probs=probs, join=grouped, dx_colsum=self.w3_colsum_target(i - 1) if i > 0 else None)
            dy, dy_b = dxo, dxo_b
            if not grouped:
                OVERLAP.join()
                yield ("block", i)
                continue
            extra = [pr._replace(dy=dy_b, Ktok=M) for pr in extra_last] if (i == 0 and hold_last and extra_last) else []
            gkey = (i, bool(self.wgrad_overwrite), len(extra), Mf, vl is not None)
            grp = ws.wgrad_groups.get(gkey)
            if grp is None:
                grp = ws.wgrad_groups[gkey] = plan_block(probs + extra, M=M, k_rows=self.m_rows, accumulate=not self.wgrad_overwrite,
                                                         device=self.store.device, scratch=self.wgrad_scratch)
            if pending is not None:
                yield ("block", pending[0])  # its weight gradients are complete (joined above)
            pending = (i, grp)
        self.held = None
        if drop:
            ops.cast_f32_bf16(dy, dy_b, M * D)
        elif pending is not None and hold_last:
            OVERLAP.run_deferred()
            self.held = pending
        elif pending is not None:  # block 0's group: nothing of this stack is left to run beside it
            pending[1].launch()
            yield ("block", pending[0])
        return dy, dy_b


# =====================================================================================================================
# RoPE tables (host, cached): exact op order of RopePositionEmbedding.forward (embeddings.py:131-180) in the dtype of
# the `periods` buffer (bf16) -- recomputing sin/cos in fp32 on the device would NOT match the reference
# =====================================================================================================================
_ROPE_CACHE: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}


def _rope_host(per: torch.Tensor, H: int, W: int, aug=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sin, cos) bf16 [H*W, 64] on the host, op for op RopePositionEmbedding.forward (embeddings.py:131-180) in the dtype of `per`.
    aug = {"shift": [2] | None, "jitter": [2] | None, "rescale": [1] | None}: the train-time coordinate augmentations (:155-171) with
    GIVEN draws (shift added per axis; jitter -- already exp() of the log-uniform draw -- multiplied per axis; rescale multiplied)."""
    dd = {"dtype": per.dtype}
    ch = torch.arange(0.5, H, **dd) / H
    cw = torch.arange(0.5, W, **dd) / W
    coords = torch.stack(torch.meshgrid(ch, cw, indexing="ij"), dim=-1).flatten(0, 1)
    coords = 2.0 * coords - 1.0
    if aug is not None:
        if aug.get("shift") is not None:
            coords += aug["shift"][None, :]
        if aug.get("jitter") is not None:
            coords *= aug["jitter"][None, :]
        if aug.get("rescale") is not None:
            coords *= aug["rescale"]
    ang = 2 * math.pi * coords[:, :, None] / per[None, None, :]
    ang = ang.flatten(1, 2).tile(2)
    return torch.sin(ang).to(torch.bfloat16).contiguous(), torch.cos(ang).to(torch.bfloat16).contiguous()


def rope_tables(periods: torch.Tensor, H: int, W: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    per = periods.detach().to("cpu")
    key = (H, W, str(device), per.dtype, tuple(per.float().tolist()))
    hit = _ROPE_CACHE.get(key)
    if hit is not None:
        return hit
    sin, cos = _rope_host(per, H, W)
    sin, cos = sin.to(device), cos.to(device)
    _ROPE_CACHE[key] = (sin, cos)
    return sin, cos


class RopeAugTabs:
    """RoPE tables of ONE list item under train-time augmentation: rows [off, off + hw) of the static per-block buffers
    sin_all / cos_all bf16 [depth, P, 64] (P = patch tokens of all items).  The trunk evaluates rope_embed inside its block loop
    (vision_transformer.py:228-233), so every block rotates with its own draw: Stack asks at(i) for block i's tables."""
    __slots__ = ("sin_all", "cos_all", "off", "hw")

    def __init__(self, sin_all, cos_all, off, hw):
        self.sin_all, self.cos_all, self.off, self.hw = sin_all, cos_all, off, hw

    def at(self, i: int):
        i = min(i, self.sin_all.shape[0] - 1)  # one shared draw for all blocks (pixel decoder): buffers [1, P, 64]
        return self.sin_all[i, self.off:self.off + self.hw], self.cos_all[i, self.off:self.off + self.hw]


def rope_at(rp, i: int):
    """(sin, cos) [hw, 64] of block i: per-block tables under augmentation, the shared pair otherwise"""
    return rp.at(i) if isinstance(rp, RopeAugTabs) else rp


def _rope_hw(rp) -> int:
    return rp.hw if isinstance(rp, RopeAugTabs) else rp[0].shape[0]


class RopeAugmenter:
    """Train-time RoPE coordinate augmentations (RopePositionEmbedding shift / jitter / rescale, embeddings.py:155-171; constructor
    arguments pos_embed_rope_*_coords of the ViT classes, reachable through the legacy YAML's vision_encoder / pixel_decoder sections):
    host-side draws in the rope dtype, tables built with the reference's op order, uploaded into STATIC device buffers that are only ever
    refreshed in place (captured hipGraph segments bake their addresses).  per_block: one draw per block and list item (trunk) or one
    per forward (pixel decoder, pixel_decoder.py:144).  An eager forward refreshes its buffer itself; under stream capture nothing
    is drawn -- the trainer calls refresh_all() before every replay."""

    def __init__(self, periods: torch.Tensor, depth: int, per_block: bool, shift, jitter, rescale, seed: int = 0):
        self.per, self.depth, self.per_block = periods.detach().to("cpu"), depth, per_block
        self.cfg = (shift, jitter, rescale)
        self.engine_id = int(seed)
        self.gen = torch.Generator().manual_seed(int(seed))
        self.records: Dict[tuple, dict] = {}
        self.touched = set()    # record keys handed out since the trainer last cleared it (what ONE captured step reads)
        self.last_draws = None  # [[draw dict per item] per block] of the latest refresh (tests replay them into the oracle)

    def reseed(self, base_seed: int, rank: int = 0):
        """the reference draws from the per-rank device RNG: data-parallel ranks must not share their augmentations.  The trainer
        calls this with its seed and rank; the stream of a (seed, rank, engine) triple is reproducible."""
        self.gen.manual_seed((int(base_seed) * 1000003 + int(rank)) * 8 + self.engine_id)

    def get_state(self) -> torch.Tensor:
        return self.gen.get_state().clone()

    def set_state(self, state: torch.Tensor):
        self.gen.set_state(state.to("cpu", torch.uint8))

    @property
    def active(self) -> bool:
        return any(v is not None for v in self.cfg)

    def _draw(self):
        import numpy as np
        shift, jitter, rescale = self.cfg
        dd = {"dtype": self.per.dtype}
        d = {"shift": None, "jitter": None, "rescale": None}
        if shift is not None:
            d["shift"] = torch.empty(2, **dd).uniform_(-shift, shift, generator=self.gen)
        if jitter is not None:
            jm = float(np.log(jitter))
            d["jitter"] = torch.empty(2, **dd).uniform_(-jm, jm, generator=self.gen).exp()
        if rescale is not None:
            rm = float(np.log(rescale))
            d["rescale"] = torch.empty(1, **dd).uniform_(-rm, rm, generator=self.gen).exp()
        return d

    def record(self, key, hws, device):
        """static buffers for a forward whose list items have (h, w) = hws"""
        rec = self.records.get(key)
        if rec is None:
            P = sum(h * w for h, w in hws)
            nb = self.depth if self.per_block else 1
            rec = dict(hws=list(hws), sin=torch.zeros(nb, P, 64, dtype=torch.bfloat16, device=device),
                       cos=torch.zeros(nb, P, 64, dtype=torch.bfloat16, device=device),
                       host=torch.zeros(2, nb, P, 64, dtype=torch.bfloat16).pin_memory(), event=None, fresh=False)
            self.records[key] = rec
        return rec

    def refresh(self, rec):
        """new draws -> host tables -> one non-blocking upload per table"""
        if rec["event"] is not None:
            rec["event"].synchronize()  # the pinned staging rows are rewritten only after the previous upload has executed
        nb = rec["sin"].shape[0]
        draws = []
        for i in range(nb):
            row, off = [], 0
            for h, w in rec["hws"]:
                d = self._draw()
                sin, cos = _rope_host(self.per, h, w, d)
                rec["host"][0, i, off:off + h * w].copy_(sin)
                rec["host"][1, i, off:off + h * w].copy_(cos)
                off += h * w
                row.append(d)
            draws.append(row)
        rec["sin"].copy_(rec["host"][0], non_blocking=True)
        rec["cos"].copy_(rec["host"][1], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        rec["event"], rec["fresh"] = ev, True
        self.last_draws = draws

    def tables(self, key, hws, device):
        """the record of this forward, refreshed unless the stream is being captured (then the trainer refreshes before each replay)"""
        rec = self.record(key, hws, device)
        self.touched.add(key)
        if torch.cuda.is_current_stream_capturing():
            if not rec["fresh"]:
                raise RuntimeError("RoPE augmentation tables must exist before stream capture (run the step eagerly once)")
        else:
            self.refresh(rec)
        return rec

    def refresh_all(self, keys=None):
        """new draws for the records a replayed graph reads (`keys`: what tables() handed out while that graph was captured; None:
        every record ever created -- host cost and one event wait per record, so the trainer passes the keys)"""
        for k, rec in self.records.items():
            if keys is None or k in keys:
                self.refresh(rec)


# =====================================================================================================================
# ViT trunk with bottleneck (vision_transformer.py:189-264, vision_transformer_bottleneck.py:48-79)
# =====================================================================================================================
class TrunkEngine:
    def __init__(self, store: ParamStore, cfg, periods: torch.Tensor, prefix: str = "trunk."):
        from .config import ffn_hidden
        self.store = store
        self.prefix = prefix  # "trunk." (student) or "teacher_trunk." (EMA teacher, vtp.py:253-268)
        self.D, self.heads, self.depth = cfg.vision_embed_dim, cfg.vision_num_heads, cfg.vision_depth
        self.H = ffn_hidden(self.D, cfg.vision_mlp_ratio, cfg.vision_ffn_layer)
        self.kind = ops.NORM_RMS if cfg.vision_norm_layer == "rmsnorm" else ops.NORM_LN
        self.eps = 1e-5 if self.kind == ops.NORM_RMS else 1e-6
        self.periods = periods.detach().to("cpu")  # host copy: rope_tables must not touch the device during graph capture
        self.pe = store.lin(self.prefix + "patch_embed.proj.weight", self.prefix + "patch_embed.proj.bias", self.D, 768)  # W^T: the input-image gradient
        self.stack = Stack(store, self.prefix + "blocks.", self.depth, self.D, self.heads, self.H, cfg.vision_norm_layer,
                           ffn=cfg.vision_ffn_layer)
        self.bott_dim = cfg.vision_feature_bottleneck
        self.bott = store.lin(self.prefix + "feature_bottleneck.weight", None, self.bott_dim, self.D) \
            if store.has(self.prefix + "feature_bottleneck.weight") else None
        # weight-gradient problems of the bottleneck on row sets other than the latent item's patch rows (the CLIP feature and the SSL
        # head rows when vision_bottleneck_ae_only=False): run by backward() in front of the latent item's own, on the main stream, so
        # that every contribution is in dW before the trunk's tail bucket is announced and no two of them write dW concurrently
        self.bott_wgrads: List[tuple] = []
        self.ws: Dict[tuple, Workspace] = {}
        # train-time RoPE coordinate augmentations (embeddings.py:155-171): one draw per block and list item
        self.rope_aug = RopeAugmenter(self.periods, self.depth, True, getattr(cfg, "vision_rope_shift_coords", None),
                                      getattr(cfg, "vision_rope_jitter_coords", None), getattr(cfg, "vision_rope_rescale_coords", None),
                                      seed=1 if prefix == "trunk." else 2)

    def workspace(self, key) -> Workspace:
        if key not in self.ws:
            self.ws[key] = Workspace(self.store.device)
        return self.ws[key]

    def forward(self, img: torch.Tensor, train: bool, masks: Optional[torch.Tensor] = None, tag: str = "", rope_aug: Optional[bool] = None,
                fp32: bool = False, keep: bool = False):
        """img f32 [B,3,H,W] -> final-norm tokens xnf bf16 [B*N, D] (N = 1 + hw).  masks: uint8 [B, hw] (1 = replace the
        patch embedding by mask_token, vision_transformer.py:194-196).  `tag` separates the buffers of passes that are in
        flight at the same time with the same shape; self.ctx() returns the handle backward() needs for such passes."""
        return self.forward_list([(img, masks)], train, tag, rope_aug=rope_aug, fp32=fp32, keep=keep)

    def tail_rows_ok(self, train: bool) -> bool:
        """may forward_list() take a tail row plan on this pass (Stack.tail_rows_ok)"""
        return self.stack.tail_rows_ok(train)

    def forward_list(self, items, train: bool, tag: str = "", rope_aug: Optional[bool] = None, tail=None, fp32: bool = False,
                     keep: bool = False):
        """items = [(img f32 [B_i,3,H_i,W_i], masks_i or None)]: the reference's list forward (forward_features_list,
        vision_transformer.py:221-258): batches of different resolution go through the blocks as ONE row-concatenated
        token buffer (one GEMM / norm launch per layer for all of them, attention + RoPE per segment).  Returns xnf bf16
        [sum_i B_i*N_i, D]; ctx().segs[i].row0 is the first row of item i.
        tail = (idx int32 [T] on the device, T, L): a row plan for the last block (Stack.forward) -- xnf then has the Mc = L + T rows
        [0, L) | L + idx[t] only (ctx().Mc; ctx().M stays the row count of the list), and so have d_xnf_buffer() and the final-norm
        backward.  Rows [0, L) keep their places: the items in front of row L are read as before."""
        st = self.store
        D = self.D
        segs, r0, p0 = [], 0, 0
        for img, masks in items:
            B, _, Hh, Ww = img.shape
            h, w = Hh // 16, Ww // 16
            sg = TrunkSeg()
            sg.B, sg.h, sg.w, sg.hw, sg.N, sg.row0, sg.prow0, sg.masks, sg.img = B, h, w, h * w, h * w + 1, r0, p0, masks, img
            sg.rope = rope_tables(self.periods, h, w, st.device)
            segs.append(sg)
            r0 += B * sg.N
            p0 += B * sg.hw
        M, P = r0, p0
        ws = self.workspace((tuple((g.B, g.h, g.w) for g in segs), tag))
        if fp32:
            if train or tail is not None:
                raise RuntimeError("TrunkEngine: the fp32 forward is an inference pass (train=False, no tail row plan)")
            return self._forward_list_fp32(ws, segs, M, keep)
        # rope_aug: None = follow `train` (RopePositionEmbedding augments when its module is in training mode); the EMA teacher's pass
        # stores nothing for a backward (train=False) but belongs to a training step: its caller passes rope_aug=True
        if self.rope_aug.active and (train if rope_aug is None else rope_aug):
            rec = self.rope_aug.tables((tuple((g.B, g.h, g.w) for g in segs), tag), [(g.h, g.w) for g in segs], st.device)
            off = 0
            for g in segs:
                g.rope = RopeAugTabs(rec["sin"], rec["cos"], off, g.hw)
                off += g.hw
        # im2col rows in the TOKEN layout (row 0 of every image is never written and stays zero): the patch-embed weight gradient is then
        # one product over the same rows as the blocks' weight gradients -- d_tokens^T patches with the cls rows contributing zero -- and
        # rides in block 0's grouped launch (backward()) instead of three few-tile split-K launches at the end of the step
        patches = ws.get("patches_tok", (M, 768), BF, zero=True)
        x0 = ws.get("x0", (M, D), F32)
        for g in segs:
            pt, xs = patches[g.row0:g.row0 + g.B * g.N], x0[g.row0:g.row0 + g.B * g.N]
            ops.im2col16_rows(g.img, pt, g.B, g.h * 16, g.w * 16, 1)
            ops.gemm_nt(pt, self.pe.w, xs, M=g.B * g.hw, N=D, K=768, bias=self.pe.bias, epi=EPI_F32, a_remap=(g.hw, 1), c_remap=(g.hw, 1))
            ops.assemble_tokens(xs, st.p(self.prefix + "cls_token"), st.p(self.prefix + "mask_token"), g.masks, g.B, g.N, D)
        stack_segs = [(g.B, g.N, g.rope) for g in segs]
        xl = self.stack.forward(ws, x0, stack_segs, 1, train, tail=tail)
        Mc = M if tail is None else tail[2] + tail[1]
        xnf = ws.get("xnf", (Mc, D), BF)
        stf = ws.get("stf", (Mc, 2), F32)
        ops.norm_fwd(xl, st.p(self.prefix + "norm.weight"), st.p(self.prefix + "norm.bias") if self.kind == ops.NORM_LN else None, xnf, stf,
                     Mc, D, self.eps, self.kind)
        c = TrunkCtx()
        c.Mc = Mc
        c.ws, c.segs, c.M, c.xl, c.xnf, c.stf, c.patches, c.stack_saved, c.x0, c.stack_segs = \
            ws, segs, M, xl, xnf, stf, patches, self.stack.last_saved, x0, stack_segs
        self._ctx = c
        return xnf

    def _forward_list_fp32(self, ws: Workspace, segs, M: int, keep: bool):
        """forward_list(train=False) in fp32 (Stack._forward_fp32): returns the final-norm tokens xnf f32 [M, D]; the ctx carries them as
        xnf32 and no bf16 xnf.  The patch-embed product runs over the token rows (the cls rows multiply zeros and are overwritten by
        assemble_tokens), in the image's own fp32 pixels."""
        st, D = self.store, self.D
        if D % 8:
            raise NotImplementedError(f"fp32 forward (trunk): vision_embed_dim must be a multiple of 8 (got {D})")
        self.stack.fp32_check("trunk")
        patches = ws.get("f32.patches_tok", (M, 768), F32, zero=True)
        x0 = ws.get("f32.x0", (M, D), F32)
        for g in segs:
            pt, xs = patches[g.row0:g.row0 + g.B * g.N], x0[g.row0:g.row0 + g.B * g.N]
            ops.im2col16_rows_f32(g.img, pt, g.B, g.h * 16, g.w * 16, 1)
            ops.gemm_nt_f32(pt, self.pe.w32, xs, M=g.B * g.N, N=D, K=768, bias=self.pe.bias)
            ops.assemble_tokens(xs, st.p(self.prefix + "cls_token"), st.p(self.prefix + "mask_token"), g.masks, g.B, g.N, D)
        stack_segs = [(g.B, g.N, g.rope) for g in segs]
        xl = self.stack.forward(ws, x0, stack_segs, 1, False, fp32=True, keep=keep)
        xnf = ws.get("f32.xnf", (M, D), F32)
        stf = ws.get("f32.stf", (M, 2), F32)
        ops.norm_fwd_f32(xl, st.p(self.prefix + "norm.weight"), st.p(self.prefix + "norm.bias") if self.kind == ops.NORM_LN else None, xnf, stf,
                         M, D, self.eps, self.kind)
        c = TrunkCtx()
        c.Mc = c.M = M
        c.ws, c.segs, c.xl, c.xnf, c.xnf32, c.stf, c.stack_segs = ws, segs, xl, None, xnf, stf, stack_segs
        self._ctx = c
        return xnf

    def latents_fp32(self, seg: int = 0) -> torch.Tensor:
        """bottleneck of the last fp32 forward on the patch rows of item `seg` -> f32 [B, hw, 64] (a view: the product runs over all token
        rows of the item, the cls rows are dropped)"""
        c = self._ctx
        g = c.segs[seg]
        R = g.B * g.N
        lat = c.ws.get("f32.lat", (R, self.bott_dim), F32)
        ops.gemm_nt_f32(c.xnf32[g.row0:g.row0 + R], self.bott.w32, lat, M=R, N=self.bott_dim, K=self.D)
        return lat.view(g.B, g.N, self.bott_dim)[:, 1:]

    def ctx(self):
        return self._ctx

    def latents(self, out_f32: bool = False, seg: int = 0) -> torch.Tensor:
        """bottleneck on the patch rows of item `seg` of the last forward -> [B*hw, 64] (bf16, or f32 for the API)."""
        c = self._ctx
        g = c.segs[seg]
        lat = c.ws.get("lat32" if out_f32 else "lat", (g.B * g.hw, self.bott_dim), F32 if out_f32 else BF)
        ops.gemm_nt(c.xnf[g.row0:], self.bott.w, lat, M=g.B * g.hw, N=self.bott_dim, K=self.D,
                    epi=EPI_F32 if out_f32 else EPI_BF16, a_remap=(g.hw, 1))
        return lat

    def bott_rows(self, x: torch.Tensor, R: int, out: torch.Tensor, lda: Optional[int] = None) -> torch.Tensor:
        """bottleneck on R arbitrary rows: out bf16 [R, 64] = x[R, D] W_bott^T (x bf16, row stride lda)"""
        ops.gemm_nt(x, self.bott.w, out, M=R, N=self.bott_dim, K=self.D, lda=x.stride(0) if lda is None else lda, epi=EPI_BF16)
        return out

    def bott_rows_bwd(self, dz: torch.Tensor, x: torch.Tensor, R: int, dx: Optional[torch.Tensor], alpha: float = 1.0):
        """backward of bott_rows: dx (bf16 [R, D], or f32 with alpha) = alpha * dz W_bott now; dW_bott += dz^T x is queued for
        backward() (self.bott_wgrads).  dz bf16 [R, 64]; x bf16 [R, D] (any row stride)."""
        if dx is not None:
            ops.gemm_nt(dz, self.bott.wT, dx, M=R, N=self.D, K=self.bott_dim, ldc=dx.stride(0),
                        epi=EPI_F32 if dx.dtype == F32 else EPI_BF16, alpha=alpha)
        self.bott_wgrads.append((dz, x, R))

    def d_xnf_buffer(self, ctx=None) -> torch.Tensor:
        """bf16 [M, D] gradient w.r.t. the final-norm tokens of the last forward (all items, row-concatenated).  The patch
        rows of the latent item are written by backward() (bottleneck dgrad); every other row must be written (or zeroed)
        by the heads before backward()."""
        c = self._ctx if ctx is None else ctx
        return c.ws.get("b.d_xnf", (c.Mc, self.D), BF, zero=True)

    def backward(self, d_lat: Optional[torch.Tensor], ctx=None, lat_seg: int = 0, want_dimg: bool = False, pool=None):
        """d_lat: bf16 [B*hw, 64] grad of latents(seg=lat_seg), or None.  Accumulates every trunk parameter gradient into
        store.flat_g.  Generator (see Stack.backward): yields "tail", then ("block", i) per block.
        pool = (seg, pvec f32 [B_seg, D]): the gradient of a mean over the patch rows of item `seg`, already divided by their count --
        added to those rows of d_xnf in f32 inside the final-norm backward (norm_bwd_pvec).
        The queued bottleneck weight-gradient problems (bott_rows_bwd) run here, in front of the latent item's own.
        want_dimg: also form the gradient w.r.t. the input images (PatchEmbed backward, embeddings.py:61-70: d_tokens[patch rows]
        W_pe folded back to pixels) -- ctx.d_img[i] f32 [B_i,3,H_i,W_i] for list item i (freshly allocated: this path is the eager
        autograd boundary, never a captured segment; the caller pops the entry -- ctx.take_d_img(i) -- so the tensor does not outlive the
        autograd call on the cached ctx); masked patches get zero (they never saw the pixels)."""
        st = self.store
        if ctx is not None:
            self._ctx = ctx
        c = self._ctx
        ws, M, D = c.ws, c.Mc, self.D  # (with a tail row plan: the compact rows; the stack's backward widens to c.M behind the last FFN)
        d_xnf = ws.get("b.d_xnf", (M, D), BF, zero=True)  # rows stay zero unless a head wrote them before backward()
        wgrads, self.bott_wgrads = self.bott_wgrads, []
        for dz, x, R in wgrads:
            linear_bwd(ws, "bott", self.bott, dz, x, R, None, need_dx=False)
        if d_lat is not None:
            g = c.segs[lat_seg]
            linear_bwd(ws, "bott", self.bott, d_lat, c.xnf[g.row0:], g.B * g.hw, d_xnf[g.row0:], x_remap=(g.hw, 1),
                       dx_remap=(g.hw, 1))
        dx = ws.get("b.dxt", (M, D), F32)
        dx_b = ws.get("b.dxt_b", (M, D), BF)
        nw, nb = st.g(self.prefix + "norm.weight"), st.g(self.prefix + "norm.bias") if self.kind == ops.NORM_LN else None
        if pool is None:
            ops.norm_bwd(d_xnf, c.xl, st.p(self.prefix + "norm.weight"), c.stf, None, dx, dx_b, nw, nb, M, D, self.kind,
                         dx_colsum=self.stack.w3_colsum_target(self.depth - 1))
        else:
            g = c.segs[pool[0]]
            ops.norm_bwd_pvec(d_xnf, c.xl, st.p(self.prefix + "norm.weight"), c.stf, None, dx, dx_b, nw, nb, M, D, self.kind, pool[1],
                              g.row0, g.B, g.N, dx_colsum=self.stack.w3_colsum_target(self.depth - 1))
        OVERLAP.join()
        yield "tail"
        g_cls, g_mask = st.g(self.prefix + "cls_token"), st.g(self.prefix + "mask_token")
        # the patch-embed weight (and bias) gradient as a fifth problem of block 0's grouped launch: dy = the stack's input gradient
        # (cls and masked rows zeroed by token_rows_bwd below, before the launch), x = the im2col rows in the token layout
        extra = [Problem(dy=None, x=c.patches, gw=self.pe.gw, gb=self.pe.gb, N=self.pe.N, K=self.pe.K, swiglu_h=0,
                         Ktok=None)] if not want_dimg and D % 8 == 0 else None  # (dy and Ktok: set where Stack.backward attaches it)
        dx0, dx0_b = yield from self.stack.backward(ws, dx, dx_b, c.stack_segs, 1, c.stack_saved,
                                                    dy_colsum_done=self.stack.w3_colsum_target(self.depth - 1) is not None,
                                                    hold_last=extra is not None, extra_last=extra)
        held, self.stack.held = self.stack.held, None
        # backward of the token assembly (vision_transformer.py:189-219): masked rows -> mask_token, row 0 -> cls_token, both zeroed in the
        # bf16 copy (what is left there is the gradient of the patch-embed output, in token rows)
        for g in c.segs:
            d_s, d_sb = dx0[g.row0:g.row0 + g.B * g.N], dx0_b[g.row0:g.row0 + g.B * g.N]
            ops.token_rows_bwd(d_s, d_sb, g.masks, g_mask if g.masks is not None else None, g_cls, g.B, g.N, D)
        if held is not None:  # (its patch-embed problem reads dx0_b)
            held[1].launch()
            yield ("block", held[0])
        else:
            for item, g in enumerate(c.segs):  # patch embed: dW += d_tokens[patch rows]^T patches, one launch sequence per item
                d_sb = dx0_b[g.row0:g.row0 + g.B * g.N]
                linear_bwd(ws, "pe", self.pe, d_sb, c.patches[g.row0:g.row0 + g.B * g.N], g.B * g.hw, None, need_dx=False,
                           dy_remap=(g.hw, 1), x_remap=(g.hw, 1))
                if want_dimg:
                    dpt = ws.get(f"b.dpatch{g.prow0}", (g.B * g.hw, 768), F32)
                    ops.gemm_nt(d_sb, self.pe.wT, dpt, M=g.B * g.hw, N=768, K=D, epi=EPI_F32, a_remap=(g.hw, 1))
                    dimg = torch.empty(g.B, 3, g.h * 16, g.w * 16, dtype=F32, device=st.device)
                    ops.col2im16(dpt, dimg, g.B, g.h * 16, g.w * 16)
                    c.__dict__.setdefault("d_img", {})[item] = dimg
        OVERLAP.join()


class TrunkSeg:
    """One item of a list forward: B images of (16h x 16w) pixels -> rows [row0, row0 + B*N) of the token buffers."""


class TrunkCtx:
    """Saved state of one trunk forward (what backward() needs)."""

    def take_d_img(self, item: int = 0):
        """the input-image gradient of list item `item` formed by backward(want_dimg=True); removes it from the ctx"""
        return self.__dict__.get("d_img", {}).pop(item)


# =====================================================================================================================
# pixel decoder (pixel_decoder.py:134-162): 1x1 conv -> blocks -> LN -> 1x1 conv -> PixelShuffle(16)
# =====================================================================================================================
class DecoderEngine:
    def __init__(self, store: ParamStore, cfg, periods: torch.Tensor):
        from .config import ffn_hidden
        self.store = store
        self.D, self.heads, self.depth = cfg.decoder_embed_dim, cfg.decoder_num_heads, cfg.decoder_depth
        self.H = ffn_hidden(self.D, 4.0, cfg.decoder_ffn_layer)
        self.kind = ops.NORM_RMS if cfg.decoder_norm_layer == "rmsnorm" else ops.NORM_LN
        self.eps = 1e-5 if self.kind == ops.NORM_RMS else 1e-6
        self.periods = periods.detach().to("cpu")
        self.cin = cfg.vision_feature_bottleneck
        self.pin = store.lin("pixel_decoder.proj_in.weight", "pixel_decoder.proj_in.bias", self.D, self.cin)
        self.stack = Stack(store, "pixel_decoder.blocks.", self.depth, self.D, self.heads, self.H, cfg.decoder_norm_layer,
                           ffn=cfg.decoder_ffn_layer)
        self.pout = store.lin("pixel_decoder.proj_out.weight", "pixel_decoder.proj_out.bias", 768, self.D)
        self.ws: Dict[tuple, Workspace] = {}
        # train-time RoPE augmentations: the decoder evaluates rope_embed ONCE per forward (pixel_decoder.py:144)
        self.rope_aug = RopeAugmenter(self.periods, self.depth, False, getattr(cfg, "decoder_rope_shift_coords", None),
                                      getattr(cfg, "decoder_rope_jitter_coords", None), getattr(cfg, "decoder_rope_rescale_coords", None), seed=3)

    def workspace(self, B, h, w) -> Workspace:
        key = (B, h, w)
        if key not in self.ws:
            self.ws[key] = Workspace(self.store.device)
        return self.ws[key]

    def forward(self, lat: torch.Tensor, B: int, h: int, w: int, train: bool, fp32: bool = False) -> torch.Tensor:
        """lat bf16 [B*hw, 64] token-major -> t bf16 [B*hw, 768] (pre-PixelShuffle, token-major).  fp32 (inference only): lat and t f32,
        every step between them in fp32 (Stack._forward_fp32)."""
        st = self.store
        M, D = B * h * w, self.D
        ws = self.workspace(B, h, w)
        if fp32:
            if train:
                raise RuntimeError("DecoderEngine: the fp32 forward is an inference pass (train=False)")
            if D % 8 or self.cin % 8:
                raise NotImplementedError(f"fp32 forward (decoder): widths must be multiples of 8 (D={D}, latent channels={self.cin})")
            self.stack.fp32_check("decoder")
            x0 = ws.get("f32.x0", (M, D), F32)
            ops.gemm_nt_f32(lat, self.pin.w32, x0, M=M, N=D, K=self.cin, bias=self.pin.bias)
            xl = self.stack.forward(ws, x0, [(B, h * w, rope_tables(self.periods, h, w, st.device))], 0, False, fp32=True)
            xnf = ws.get("f32.xnf", (M, D), F32)
            ops.norm_fwd_f32(xl, st.p("pixel_decoder.norm.weight"), st.p("pixel_decoder.norm.bias") if self.kind == ops.NORM_LN else None,
                             xnf, ws.get("f32.stf", (M, 2), F32), M, D, self.eps, self.kind)
            t = ws.get("f32.t", (M, 768), F32)
            ops.gemm_nt_f32(xnf, self.pout.w32, t, M=M, N=768, K=D, bias=self.pout.bias)
            return t
        x0 = ws.get("x0", (M, D), F32)
        ops.gemm_nt(lat, self.pin.w, x0, M=M, N=D, K=self.cin, bias=self.pin.bias, epi=EPI_F32)
        rope = rope_tables(self.periods, h, w, st.device)
        if train and self.rope_aug.active:
            rec = self.rope_aug.tables((B, h, w), [(h, w)], st.device)
            # (RopeAugTabs, not a plain pair: _rope_plan keeps a COPY of plain tables, keyed by their address -- a buffer that is
            # refreshed in place would leave the fused qkv + RoPE epilogue rotating with the first step's draw)
            rope = RopeAugTabs(rec["sin"], rec["cos"], 0, h * w)
        segs = [(B, h * w, rope)]
        xl = self.stack.forward(ws, x0, segs, 0, train)
        xnf = ws.get("xnf", (M, D), BF)
        stf = ws.get("stf", (M, 2), F32)
        ops.norm_fwd(xl, st.p("pixel_decoder.norm.weight"),
                     st.p("pixel_decoder.norm.bias") if self.kind == ops.NORM_LN else None, xnf, stf, M, D, self.eps, self.kind)
        t = ws.get("t", (M, 768), BF)
        ops.gemm_nt(xnf, self.pout.w, t, M=M, N=768, K=D, bias=self.pout.bias, epi=EPI_BF16)
        self._ctx = (ws, B, h, w, lat, xl, xnf, stf, segs, self.stack.last_saved)
        return t

    def backward(self, dt: torch.Tensor):
        """dt bf16 [B*hw, 768] -> d_lat bf16 [B*hw, 64]; parameter grads accumulate into store.flat_g.
        Generator: yields "tail", then ("block", i) per block; returns d_lat."""
        st = self.store
        ws, B, h, w, lat, xl, xnf, stf, segs, stack_saved = self._ctx
        M, D = B * h * w, self.D
        d_xnf = ws.get("b.d_xnf", (M, D), BF)
        linear_bwd(ws, "pout", self.pout, dt, xnf, M, d_xnf)
        dx = ws.get("b.dxt", (M, D), F32)
        dx_b = ws.get("b.dxt_b", (M, D), BF)
        ops.norm_bwd(d_xnf, xl, st.p("pixel_decoder.norm.weight"), stf, None, dx, dx_b, st.g("pixel_decoder.norm.weight"),
                     st.g("pixel_decoder.norm.bias") if self.kind == ops.NORM_LN else None, M, D, self.kind,
                     dx_colsum=self.stack.w3_colsum_target(self.depth - 1))
        OVERLAP.join()
        yield "tail"
        dx0, dx0_b = yield from self.stack.backward(ws, dx, dx_b, segs, 0, stack_saved,
                                                    dy_colsum_done=self.stack.w3_colsum_target(self.depth - 1) is not None)
        d_lat = ws.get("b.d_lat", (M, self.cin), BF)
        linear_bwd(ws, "pin", self.pin, dx0_b, lat, M, d_lat)
        OVERLAP.join()
        return d_lat
