"""CLIP side of the VTP hot path on the gfx950 kernels: text tower (TextTransformer pieces as re-hung by
VTPModel._init_text_components, modeling_vtp.py:135-178) and the image/text projection + normalisation heads
(modeling_vtp.py:244-333).  The contrastive loss itself is our spec (OpenCLIP convention, parity unpinned)."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import ops
from .engine import BF, F32, OVERLAP, ParamStore, RowPlan, Stack, Workspace, _env_flag, linear_bwd
from .ops import EPI_BF16, EPI_F32

I32 = torch.int32


class TextEngine:
    def __init__(self, store: ParamStore, cfg):
        self.store = store
        self.D, self.heads, self.depth, self.T = cfg.text_embed_dim, cfg.text_num_heads, cfg.text_depth, cfg.text_num_pos
        self.H = int(self.D * cfg.text_mlp_ratio)
        self.Dout = cfg.text_embed_dim  # output_dim = text_embed_dim (modeling_vtp.py:150)
        self.stack = Stack(store, "text_transformer.resblocks.", self.depth, self.D, self.heads, self.H, "layernorm",
                           style="text")
        # text_transformer.py:285-288: no_causal_mask drops the additive causal mask (full attention over the T tokens);
        # text_global_pool (:213-228): the pooled row is the first / last token or the arg-max id (EOT) of every caption
        self.stack.causal = not cfg.text_no_causal_mask
        self.stack.quick_gelu = bool(cfg.text_quick_gelu)  # act_layer = QuickGELU (modeling_vtp.py:139)
        self.pool = cfg.text_pool_type
        # Packed captions: under the causal mask no row up to a caption's EOT depends on a row behind it, and arg-max pooling reads the EOT
        # row alone -- so the rows behind it are dead in the forward and receive exact zeros in the backward.  The tower then runs on the
        # live rows only, stored back to back; their count stays on the device (ops.text_row_plan), so launch shapes and a captured graph
        # are those of B * T rows.  Every other variant (no causal mask, first / last / none pooling, text_embed_cls) keeps all rows;
        # VTP_TEXT_VARLEN=0 forces that path (same-box A/B runs).
        self.packed = self.stack.causal and self.pool == "argmax" and not cfg.text_embed_cls
        # text_projection is stored [width, output_dim] and applied as x @ P (modeling_vtp.py:308): as a Lin with
        # N = width, K = output_dim its bf16 copy `w` is P and `wT` is P^T (the K-contiguous operand of the forward GEMM)
        self.proj = store.lin("text_projection", None, self.D, self.Dout)
        self.projT32 = None  # fp32 forward: P^T f32 [Dout, D], derived data (enable_fp32), refreshed with the bf16 copies
        self.ws: Dict[tuple, Workspace] = {}

    def workspace(self, B) -> Workspace:
        if B not in self.ws:
            self.ws[B] = Workspace(self.store.device)
        return self.ws[B]

    def enable_fp32(self):
        """derive what the fp32 forward needs beyond the masters: the K-contiguous transpose of text_projection.  Rebuilt wherever the
        bf16 copies are (a ParamStore prep hook)."""
        self.stack.fp32_check("text")
        if self.D % 8 or self.Dout % 8:
            raise NotImplementedError(f"fp32 forward (text): text_embed_dim must be a multiple of 8 (got {self.D})")
        if self.projT32 is None:
            self.projT32 = torch.empty(self.Dout, self.D, dtype=F32, device=self.store.device)
            if not hasattr(self.store, "prep_hooks"):
                self.store.prep_hooks = []
            self.store.prep_hooks.append(self._refresh_fp32)
        self._refresh_fp32()

    def _refresh_fp32(self):
        self.projT32.copy_(self.proj.w32.t())

    def _forward_fp32(self, ids: torch.Tensor) -> torch.Tensor:
        """forward(train=False) in fp32: all B * T rows (no packed captions), Stack._forward_fp32, ln_final and the projection in fp32"""
        st, D = self.store, self.D
        B, T = ids.shape
        if self.projT32 is None:
            raise RuntimeError("TextEngine: the fp32 forward was not enabled (enable_fp32)")
        ws = self.workspace(B)
        x0 = ws.get("f32.x0", (B * T, D), F32)
        eot = ws.get("f32.eot", (B,), I32)
        self.stack.varlen = None
        ops.embed_tokens(ids, st.p("token_embedding.weight"), st.p("positional_embedding"), x0, eot, B, T, D)
        if self.pool in ("first", "last"):
            eot.fill_(0 if self.pool == "first" else T - 1)
        xl = self.stack.forward(ws, x0, [(B, T, None)], 0, False, fp32=True)
        R = B * T
        if self.pool != "none":  # ln_final is row-wise: pool first
            R = B
            pooled = ws.get("f32.pooled", (B, D), F32)
            ops.gather_rows(xl, eot, pooled, B, T, D)
            xl = pooled
        xn = ws.get("f32.xn_final", (R, D), F32)
        ops.norm_fwd_f32(xl, st.p("ln_final.weight"), st.p("ln_final.bias"), xn, ws.get("f32.stf", (R, 2), F32), R, D, 1e-5, ops.NORM_LN)
        feat = ws.get("f32.feat", (R, self.Dout), F32)
        ops.gemm_nt_f32(xn, self.projT32, feat, M=R, N=self.Dout, K=D)
        return feat

    def forward(self, ids: torch.Tensor, train: bool, fp32: bool = False) -> torch.Tensor:
        """ids int64 [B, T] (device) -> un-normalised text features f32 [B, Dout]  (modeling_vtp.py:278-310); text_pool_type = "none"
        (text_global_pool's fall-through, text_transformer.py:225-226): every token, f32 [B * T, Dout]."""
        if fp32:
            if train:
                raise RuntimeError("TextEngine: the fp32 forward is an inference pass (train=False)")
            return self._forward_fp32(ids)
        st = self.store
        B, T = ids.shape
        D = self.D
        ws = self.workspace(B)
        x0 = ws.get("x0", (B * T, D), F32)
        eot = ws.get("eot", (B,), I32)
        plan = None
        if self.packed and _env_flag("VTP_TEXT_VARLEN") and self.stack.varlen_ok(B * T):
            plan = RowPlan(ws.get("cu", (B + 1,), I32), ws.get("rows", (1,), I32))
        self.stack.varlen = plan
        if plan is not None:
            cu, rows = plan
            ops.text_row_plan(ids, eot, cu, rows, B, T)
            ops.embed_tokens_packed(ids, st.p("token_embedding.weight"), st.p("positional_embedding"), x0, cu, B, T, D)
            xl = self.stack.forward(ws, x0, [(B, T, None)], 0, train)
            pooled = ws.get("pooled", (B, D), F32)
            ops.gather_rows_packed(xl, cu, pooled, B, D)
            return self._head(ws, ids, B, T, eot, pooled, plan)
        ops.embed_tokens(ids, st.p("token_embedding.weight"), st.p("positional_embedding"), x0, eot, B, T, D)
        if self.pool in ("first", "last"):  # the kernel wrote the arg-max position of every row; 'first' / 'last' pool a fixed position
            eot.fill_(0 if self.pool == "first" else T - 1)
        xl = self.stack.forward(ws, x0, [(B, T, None)], 0, train)
        if self.pool == "none":  # ln_final and the projection over all B * T rows
            xn = ws.get("all_n", (B * T, D), BF)
            stf = ws.get("all_stf", (B * T, 2), F32)
            ops.norm_fwd(xl, st.p("ln_final.weight"), st.p("ln_final.bias"), xn, stf, B * T, D, 1e-5, ops.NORM_LN)
            feat = ws.get("all_feat", (B * T, self.Dout), F32)
            ops.gemm_nt(xn, self.proj.wT, feat, M=B * T, N=self.Dout, K=D, epi=EPI_F32)
            self._ctx = (ws, ids, B, T, None, xl, xn, stf, None)
            return feat
        pooled = ws.get("pooled", (B, D), F32)
        ops.gather_rows(xl, eot, pooled, B, T, D)  # ln_final is row-wise: pool first, normalise B rows instead of B*T
        return self._head(ws, ids, B, T, eot, pooled, None)

    def _head(self, ws, ids, B, T, eot, pooled, plan):
        """ln_final and the projection of the B pooled rows"""
        st, D = self.store, self.D
        pn = ws.get("pooled_n", (B, D), BF)
        stf = ws.get("stf", (B, 2), F32)
        ops.norm_fwd(pooled, st.p("ln_final.weight"), st.p("ln_final.bias"), pn, stf, B, D, 1e-5, ops.NORM_LN)
        feat = ws.get("feat", (B, self.Dout), F32)
        ops.gemm_nt(pn, self.proj.wT, feat, M=B, N=self.Dout, K=D, epi=EPI_F32)
        self._ctx = (ws, ids, B, T, eot, pooled, pn, stf, plan)
        return feat

    def backward(self, d_feat: torch.Tensor):
        """d_feat f32 [B, Dout].  Generator (see Stack.backward): yields "tail" then ("block", i); parameter gradients
        accumulate into store.flat_g."""
        st = self.store
        ws, ids, B, T, eot, pooled, pn, stf, plan = self._ctx
        D = self.D
        self.stack.varlen = plan  # (the forward's: another forward may have run since)
        if eot is None:  # text_pool_type = "none": the same head over all B * T rows, no pooling scatter
            R = B * T
            d_feat_b = ws.get("b.all_d_feat_b", (R, self.Dout), BF)
            ops.cast_f32_bf16(d_feat, d_feat_b, R * self.Dout)
            linear_bwd(ws, "tproj", None, pn, d_feat_b, R, None, need_dx=False, N=D, K=self.Dout, gw=self.proj.gw, gb=None, wT=None)
            d_pn = ws.get("b.all_d_pn", (R, D), BF)
            ops.gemm_nt(d_feat_b, self.proj.w, d_pn, M=R, N=D, K=self.Dout, epi=EPI_BF16)
            dx = ws.get("b.dxt", (R, D), F32)
            dx_b = ws.get("b.dxt_b", (R, D), BF)
            ops.norm_bwd(d_pn, pooled, st.p("ln_final.weight"), stf, None, dx, dx_b, st.g("ln_final.weight"), st.g("ln_final.bias"), R, D,
                         ops.NORM_LN)
            OVERLAP.join()
            yield "tail"
            dx0, _ = yield from self.stack.backward(ws, dx, dx_b, [(B, T, None)], 0)
            ops.embed_tokens_bwd(ids, dx0, st.g("token_embedding.weight"), st.g("positional_embedding"), B, T, D)
            OVERLAP.join()
            return
        d_feat_b = ws.get("b.d_feat_b", (B, self.Dout), BF)
        ops.cast_f32_bf16(d_feat, d_feat_b, B * self.Dout)
        # dP [D, Dout] += pn^T d_feat  (roles of "dy" and "x" swapped so the result lands in the parameter's layout)
        linear_bwd(ws, "tproj", None, pn, d_feat_b, B, None, need_dx=False, N=D, K=self.Dout, gw=self.proj.gw, gb=None,
                   wT=None)
        d_pn = ws.get("b.d_pn", (B, D), BF)
        ops.gemm_nt(d_feat_b, self.proj.w, d_pn, M=B, N=D, K=self.Dout, epi=EPI_BF16)  # d_pn = d_feat P^T
        d_pooled = ws.get("b.d_pooled", (B, D), F32)
        ops.norm_bwd(d_pn, pooled, st.p("ln_final.weight"), stf, None, d_pooled, None, st.g("ln_final.weight"),
                     st.g("ln_final.bias"), B, D, ops.NORM_LN)
        dx = ws.get("b.dxt", (B * T, D), F32)
        dx_b = ws.get("b.dxt_b", (B * T, D), BF)
        if plan is not None:
            ops.scatter_rows_packed(d_pooled, plan.cu, dx, dx_b, B, T, D)
        else:
            ops.scatter_rows(d_pooled, eot, dx, dx_b, B, T, D)
        OVERLAP.join()
        yield "tail"
        dx0, _ = yield from self.stack.backward(ws, dx, dx_b, [(B, T, None)], 0)
        if plan is not None:
            ops.embed_tokens_bwd_packed(ids, dx0, st.g("token_embedding.weight"), st.g("positional_embedding"), plan.cu, B, T, D)
        else:
            ops.embed_tokens_bwd(ids, dx0, st.g("token_embedding.weight"), st.g("positional_embedding"), B, T, D)
        OVERLAP.join()


class ClipHead:
    """visual_proj + F.normalize on both modalities + contrastive loss with (optional) cross-rank feature exchange."""

    def __init__(self, store: ParamStore, vproj, Dv: int, Dt: int, feat: str = "cls", trunk=None):
        """feat: vision_clip_feat ('cls' | 'pooled': the cls token or the mean of the patch tokens, modeling_vtp.py:261-276); trunk: the
        TrunkEngine whose feature_bottleneck the feature goes through first (vision_bottleneck_ae_only=False), or None"""
        if feat not in ("cls", "pooled"):
            raise ValueError(f"vision_clip_feat must be 'cls' or 'pooled', got {feat!r}")
        self.store, self.vproj, self.Dv, self.Dt, self.feat, self.trunk = store, vproj, Dv, Dt, feat, trunk
        assert vproj.K == (trunk.bott_dim if trunk is not None else Dv), "visual_proj input width does not match the CLIP feature"
        self.ws = Workspace(store.device)

    def image_features(self, xnf: torch.Tensor, B: int, N: int) -> torch.Tensor:
        """final-norm token rows of one list item (bf16 [B*N, Dv], image b = rows b*N..) -> un-normalised image features f32 [B, Dt]:
        the cls row or the mean of the patch rows (one pool_patch_rows launch), through the bottleneck when there is one, then
        visual_proj (B-row GEMMs; the bottleneck of the pooled feature is applied after the mean: it is linear)."""
        ws, D = self.ws, self.Dv
        if self.feat == "cls":
            x, lda = xnf, N * D  # strided rows: row b = token b*N
        else:
            pooled = ws.get(f"pool{B}", (B, D), F32)
            ops.pool_patch_rows(xnf, pooled, B, N, D)
            x = ws.get(f"pool_b{B}", (B, D), BF)
            ops.cast_f32_bf16(pooled, x, B * D)
            lda = D
        self._x = (x, lda)
        if self.trunk is not None:
            z = self.trunk.bott_rows(x, B, ws.get(f"z{B}", (B, self.trunk.bott_dim), BF), lda=lda)
            x, lda = z, z.stride(0)
        self._in = x
        f = ws.get(f"f_img{B}", (B, self.Dt), F32)
        ops.gemm_nt(x, self.vproj.w, f, M=B, N=self.Dt, K=self.vproj.K, lda=lda, epi=EPI_F32)
        return f

    def image_features_fp32(self, xnf: torch.Tensor, B: int, N: int) -> torch.Tensor:
        """image_features on the fp32 forward's token rows (f32 [B*N, Dv]), every product in fp32"""
        ws, D = self.ws, self.Dv
        if self.feat == "cls":
            x, lda = xnf, N * D
        else:
            x = ws.get(f"f32.pool{B}", (B, D), F32)
            ops.pool_patch_rows_f32(xnf, x, B, N, D)
            lda = D
        K = D
        if self.trunk is not None:
            K = self.trunk.bott_dim
            z = ws.get(f"f32.z{B}", (B, K), F32)
            ops.gemm_nt_f32(x, self.trunk.bott.w32, z, M=B, N=K, K=D, lda=lda)
            x, lda = z, K
        f = ws.get(f"f32.f_img{B}", (B, self.Dt), F32)
        ops.gemm_nt_f32(x, self.vproj.w32, f, M=B, N=self.Dt, K=K, lda=lda)
        return f

    def normalize(self, f: torch.Tensor, tag: str):
        B, D = f.shape
        y = self.ws.get(f"n_{tag}{B}", (B, D), F32)
        inv = self.ws.get(f"inv_{tag}{B}", (B,), F32)
        ops.l2norm_fwd(f, y, inv, B, D, 1e-12)
        return y, inv

    def normalize_bwd(self, dy, y, inv, tag: str):
        B, D = y.shape
        dx = self.ws.get(f"dn_{tag}{B}", (B, D), F32)
        ops.l2norm_bwd(dy, y, inv, dx, B, D)
        return dx

    def image_backward(self, d_f: torch.Tensor, xnf: torch.Tensor, d_xnf: torch.Tensor, B: int, N: int) -> Optional[torch.Tensor]:
        """d_f f32 [B, Dt] -> dW(visual_proj) and the feature's gradient: cls feature -- written to the cls rows of d_xnf (bf16
        [B*N, Dv]); pooled feature -- returned as the per-image vector f32 [B, Dv] (already divided by the N - 1 patch rows) that the
        trunk's final-norm backward adds to every patch row (TrunkEngine.backward(pool=...)).  Through the bottleneck, its weight
        gradient is queued on the trunk (TrunkEngine.bott_rows_bwd)."""
        ws, D = self.ws, self.Dv
        if self.feat == "pooled" and D > 1024:  # (the final-norm backward that takes the pooled gradient: rows up to 1024 wide)
            raise NotImplementedError(f"the fused step with vision_clip_feat='pooled' needs vision_embed_dim <= 1024 (got {D})")
        d_f_b = ws.get(f"d_f_b{B}", (B, self.Dt), BF)
        ops.cast_f32_bf16(d_f, d_f_b, B * self.Dt)
        cls_rows = xnf.view(B, N * D)[:, :D]        # strided views: row b = token b*N
        d_cls_rows = d_xnf.view(B, N * D)[:, :D]
        tr = self.trunk
        if tr is None and self.feat == "cls":
            linear_bwd(ws, "vproj", self.vproj, d_f_b, cls_rows, B, d_cls_rows)
            return None
        pvec = ws.get(f"pvec{B}", (B, D), F32) if self.feat == "pooled" else None
        x = cls_rows if self.feat == "cls" else self._x[0]
        if tr is None:  # pooled, un-bottlenecked: d_pooled / (N - 1) = d_f Wv / (N - 1)
            linear_bwd(ws, "vproj", self.vproj, d_f_b, x, B, None, need_dx=False)
            ops.gemm_nt(d_f_b, self.vproj.wT, pvec, M=B, N=D, K=self.Dt, epi=EPI_F32, alpha=1.0 / (N - 1))
            return pvec
        dz = ws.get(f"dz{B}", (B, tr.bott_dim), BF)
        linear_bwd(ws, "vproj", self.vproj, d_f_b, self._in, B, dz)
        if self.feat == "cls":
            tr.bott_rows_bwd(dz, x, B, d_cls_rows)
        else:  # the pooled latent's gradient g enters every patch row as (g W_bott) / (N - 1); dW_bott += g^T mean(patch rows)
            tr.bott_rows_bwd(dz, x, B, pvec, alpha=1.0 / (N - 1))
        return pvec
