"""Host-side refusals of the entry points that share a launcher (norm, tiled attention, grouped 8-phase wgrad, GELU backward): every
case below is rejected with VTP_ERR_ARG before any HIP call, so it runs without a GPU, and the message names the entry point the
caller used and the limit it broke.  Nothing here gets through validation -- an accepted call would try to launch."""
import ctypes

import pytest

P = ctypes.c_void_p(16)  # a non-null pointer; a refused call dereferences nothing
N = None


def norm_fwd(D=768, M=8, kind=0, x=P, b=P):
    return (x, P, b, P, P, M, D, 1e-6, kind, N)


def norm_fwd_limit(D=768, M=8, kind=0, x=P, b=P, m_rows=P):
    return (x, P, b, P, P, M, D, 1e-6, kind, m_rows, N)


def norm_fwd_e4m3(D=768, M=8, kind=0, x=P, b=P, q_scale=P):
    return (x, P, b, P, q_scale, P, M, D, 1e-6, kind, N)


def norm_bwd(D=768, M=8, kind=0, dy=P, dxb=P, dxsum=P):
    return (dy, P, P, P, P, P, dxb, P, P, dxsum, M, D, kind, N)


def norm_bwd_limit(D=768, M=8, kind=0, dy=P, dxb=P, dxsum=P, m_rows=P):
    return (dy, P, P, P, P, P, dxb, P, P, dxsum, M, D, kind, m_rows, N)


def norm_bwd_pvec(D=768, M=8, kind=0, dy=P, dxb=P, dxsum=P, pvec=P, prow0=0, pB=2, pN=4):
    return (dy, P, P, P, P, P, dxb, P, P, dxsum, pvec, prow0, pB, pN, M, D, kind, N)


def norm_bwd_rows(D=768, M=8, kind=0, dy=P, dxb=P, dxsum=P, dres=P, rows=P, dres_M=4):
    return (dy, P, P, P, dres, rows, dres_M, P, dxb, P, P, dxsum, M, D, kind, N)


def attn_fwd(q=P, B=2, n=512, heads=4, sn=768, causal=0):
    return (q, P, P, P, P, B, n, heads, n * sn, sn, n * 256, 256, 0.125, causal, N)


def attn_bwd(q=P, B=2, n=512, heads=4, sn=768, causal=0, rsin=N, rcos=N, prefix=0):
    return (q, P, P, P, P, P, P, P, P, P, rsin, rcos, prefix, B, n, heads, n * sn, sn, n * 256, 256, 0.125, causal, N)


def attn_fwd_varlen(q=P, cu=P, B=2, n=77, heads=4, sn=768):
    return (q, P, P, P, P, cu, B, n, heads, sn, 256, 0.125, N)


def attn_bwd_varlen(q=P, cu=P, B=2, n=77, heads=4, sn=768):
    return (q, P, P, P, P, P, P, P, P, P, cu, B, n, heads, sn, 256, 0.125, N)


def grouped(probs=P, nprob=4, ntiles=12, K=512, splits=1, part=N, ticket=N):
    return (probs, nprob, ntiles, K, splits, part, ticket, N)


def grouped_limit(probs=P, nprob=4, ntiles=12, K=512, k_rows=P):
    return (probs, nprob, ntiles, K, k_rows, N)


def gelu(dy=P, n=64):
    return (dy, P, P, n, N)


def gelu_limit(dy=P, M=8, H=64, quick=0, m_rows=P):
    return (dy, P, P, M, H, quick, m_rows, N)


NORM_FWD = [("vtp_norm_fwd", norm_fwd), ("vtp_norm_fwd_limit", norm_fwd_limit), ("vtp_norm_fwd_e4m3", norm_fwd_e4m3)]
NORM_BWD = [("vtp_norm_bwd", norm_bwd), ("vtp_norm_bwd_limit", norm_bwd_limit), ("vtp_norm_bwd_pvec", norm_bwd_pvec),
            ("vtp_norm_bwd_rows", norm_bwd_rows)]
ATTN = [("vtp_attn_fwd", attn_fwd), ("vtp_attn_bwd", attn_bwd), ("vtp_attn_fwd_varlen", attn_fwd_varlen),
        ("vtp_attn_bwd_varlen", attn_bwd_varlen)]

# (entry point, arguments, token the message must contain)
CASES = []
for name, mk in NORM_FWD:
    CASES += [(name, mk(x=N), "null"), (name, mk(D=2052), "2048"), (name, mk(D=770), "% 4"), (name, mk(D=0), "2048"),
              (name, mk(M=0), "2048"), (name, mk(kind=2), "kind"), (name, mk(kind=1, b=N), "kind")]
CASES += [("vtp_norm_fwd_limit", norm_fwd_limit(m_rows=N), "null"), ("vtp_norm_fwd_e4m3", norm_fwd_e4m3(q_scale=N), "null")]
for name, mk in NORM_BWD:
    # (M = 0 also empties the pooled-vector segment range, so that entry may name either limit)
    CASES += [(name, mk(dy=N), "null"), (name, mk(D=2052), "D <="), (name, mk(D=770), "% 4"),
              (name, mk(M=0), "" if name == "vtp_norm_bwd_pvec" else "D <="), (name, mk(kind=2), "kind"), (name, mk(dxb=N), "dx_colsum")]
CASES += [
    # the pooled-vector and row-map variants have no instantiation for rows wider than 1024; their siblings go to 2048
    ("vtp_norm_bwd_pvec", norm_bwd_pvec(D=1028), "1024"),
    ("vtp_norm_bwd_rows", norm_bwd_rows(D=1028), "1024"),
    ("vtp_norm_bwd", norm_bwd(D=2052), "2048"),
    ("vtp_norm_bwd_limit", norm_bwd_limit(D=2052), "2048"),
    ("vtp_norm_bwd_limit", norm_bwd_limit(m_rows=N), "null"),
    ("vtp_norm_bwd_pvec", norm_bwd_pvec(pvec=N), "null"),
    ("vtp_norm_bwd_pvec", norm_bwd_pvec(prow0=4), "segment"),  # rows [4, 4 + 2*4) leave M = 8
    ("vtp_norm_bwd_pvec", norm_bwd_pvec(pN=1), "segment"),
    ("vtp_norm_bwd_pvec", norm_bwd_pvec(prow0=-1), "segment"),
    ("vtp_norm_bwd_rows", norm_bwd_rows(dres=N), "needs dres"),
    ("vtp_norm_bwd_rows", norm_bwd_rows(dres_M=0), "dres_M"),
    # without a row map vtp_norm_bwd_rows is vtp_norm_bwd, whose width limit is 2048
    ("vtp_norm_bwd_rows", norm_bwd_rows(rows=N, D=2052), "2048"),
]
for name, mk in ATTN:
    CASES += [(name, mk(q=N), "null"), (name, mk(B=0), "bad shape"), (name, mk(n=0), "bad shape"), (name, mk(heads=0), "bad shape"),
              (name, mk(sn=772), "multiples of 8"), (name, mk(B=65536), "65535"), (name, mk(heads=65536), "65535")]
CASES += [
    ("vtp_attn_fwd_varlen", attn_fwd_varlen(cu=N), "null"),
    ("vtp_attn_bwd_varlen", attn_bwd_varlen(cu=N), "null"),
    ("vtp_attn_bwd", attn_bwd(rsin=P), "go together"),
    ("vtp_attn_bwd", attn_bwd(rsin=P, rcos=P, prefix=513), "rope_prefix"),
    ("vtp_gemm_tn_grouped", grouped(probs=N), "1..8 problems"),
    ("vtp_gemm_tn_grouped", grouped(nprob=0), "1..8 problems"),
    ("vtp_gemm_tn_grouped", grouped(nprob=9), "1..8 problems"),
    ("vtp_gemm_tn_grouped", grouped(ntiles=0), "bad shape"),
    ("vtp_gemm_tn_grouped", grouped(K=0), "bad shape"),
    ("vtp_gemm_tn_grouped", grouped(splits=0), "bad shape"),
    ("vtp_gemm_tn_grouped", grouped(splits=2), "split-K"),
    ("vtp_gemm_tn_grouped", grouped(splits=2, part=P), "split-K"),
    ("vtp_gemm_tn_grouped_limit", grouped_limit(probs=N), "1..8 problems"),
    ("vtp_gemm_tn_grouped_limit", grouped_limit(k_rows=N), "row count"),
    ("vtp_gemm_tn_grouped_limit", grouped_limit(nprob=9), "1..8 problems"),
    ("vtp_gemm_tn_grouped_limit", grouped_limit(ntiles=0), "bad shape"),
    ("vtp_gemm_tn_grouped_limit", grouped_limit(K=0), "bad shape"),
]
for name in ("vtp_gelu_bwd", "vtp_quick_gelu_bwd"):
    CASES += [(name, gelu(dy=N), "bad argument"), (name, gelu(n=12), "% 8"), (name, gelu(n=0), "% 8")]
CASES += [
    ("vtp_gelu_bwd_limit", gelu_limit(dy=N), "bad argument"),
    ("vtp_gelu_bwd_limit", gelu_limit(m_rows=N), "bad argument"),
    ("vtp_gelu_bwd_limit", gelu_limit(H=12), "% 8"),
    ("vtp_gelu_bwd_limit", gelu_limit(M=0), "% 8"),
    ("vtp_gelu_bwd_limit", gelu_limit(H=12, quick=1), "% 8"),
]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    return _lib.load()


def test_every_shared_launcher_entry_has_a_null_and_a_shape_case():
    names = {c[0] for c in CASES}
    assert len(names) == 16
    for name in names:
        tokens = [c[2] for c in CASES if c[0] == name]
        assert any(t in ("null", "bad argument", "1..8 problems") for t in tokens), name
        assert any(t not in ("null", "bad argument") for t in tokens), name


@pytest.mark.parametrize("name,args,token", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_refused_before_any_hip_call(lib, name, args, token):
    rc = getattr(lib, name)(*args)
    msg = lib.vtp_last_error().decode()
    assert rc == -1, f"{name}: rc {rc}"
    # the message starts with the entry point the caller used -- except through vtp_norm_bwd_rows without a row map, which IS
    # vtp_norm_bwd and says so
    who = "vtp_norm_bwd" if name == "vtp_norm_bwd_rows" and args[5] is None else name
    assert msg.startswith(who + ":"), msg
    assert token in msg, msg


@pytest.mark.parametrize("name,mk", NORM_BWD[:2])
def test_plain_and_limit_norm_bwd_do_not_refuse_d_1028_for_its_width(lib, name, mk):
    """D = 1028 is a legal width for the plain and the row-limit backward (only the pooled-vector and row-map variants stop at 1024):
    with a null dy on top, the refusal is the null-pointer one and does not mention a width."""
    rc = getattr(lib, name)(*mk(D=1028, dy=N))
    msg = lib.vtp_last_error().decode()
    assert rc == -1 and msg.startswith(name + ":") and "null" in msg, msg
    assert "1024" not in msg and "1028" not in msg and "2048" not in msg, msg
