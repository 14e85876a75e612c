"""Host-side refusals of the fp8 (e4m3) entry points, in the manner of tests/test_launchers_host.py: every case below is rejected with
VTP_ERR_ARG before any HIP call, so it runs without a GPU on dummy pointers, and the message names the entry point and the limit."""
import ctypes

import pytest

P = ctypes.c_void_p(16)   # a non-null, 16-byte aligned pointer; a refused call dereferences nothing
Q = ctypes.c_void_p(24)   # a misaligned one
N = None
BF16, F32, SWIGLU, GELU, F32_ATOMIC, F32_SLAB = 0, 1, 2, 3, 4, 5


def gemm(A=P, lda=None, B=P, ldb=None, C=P, ldc=None, bias=P, M=64, Nn=256, K=128, epi=BF16, rope=(N, N, N, 0)):
    return (A, K if lda is None else lda, B, K if ldb is None else ldb, C, Nn if ldc is None else ldc, N, 0, bias, N, M, Nn, K, epi, 1.0,
            *rope, N)


def quant(src=P, dst=P, n=64):
    return (src, 0, dst, n, N, 1.0, N)


def amax(src=P, out=P, n=64):
    return (src, 0, n, out, N)


def dequant(src=P, dst=P, n=64):
    return (src, dst, n, 1.0, N)


G = "vtp_gemm_nt_fp8"
# (entry point, arguments, token the message must contain)
CASES = [
    (G, gemm(A=N), "null"), (G, gemm(B=N), "null"), (G, gemm(C=N), "null"),
    (G, gemm(M=0), "bad shape"), (G, gemm(Nn=0, ldc=256), "bad shape"), (G, gemm(K=0, lda=128, ldb=128), "bad shape"),
    (G, gemm(K=120), "multiples of 16"), (G, gemm(lda=136), "multiples of 16"), (G, gemm(ldb=136), "multiples of 16"),
    (G, gemm(Nn=258, ldc=260), "multiples of 4"), (G, gemm(ldc=258), "multiples of 4"),
    (G, gemm(A=Q), "16-B aligned"), (G, gemm(B=Q), "16-B aligned"), (G, gemm(C=Q), "16-B aligned"),
    (G, gemm(epi=GELU), "forward epilogues"), (G, gemm(epi=F32_ATOMIC), "forward epilogues"), (G, gemm(epi=F32_SLAB), "forward epilogues"),
    (G, gemm(epi=SWIGLU, bias=N), "SwiGLU"), (G, gemm(epi=SWIGLU, Nn=264), "SwiGLU"),
    (G, gemm(epi=F32, rope=(P, P, P, 128)), "RoPE"), (G, gemm(rope=(P, N, P, 128)), "RoPE"), (G, gemm(rope=(P, P, N, 128)), "RoPE"),
    (G, gemm(rope=(P, P, P, 64)), "% 128"), (G, gemm(rope=(P, P, P, 384)), "rope_cols <= N"),
    # 32-bit staging offsets: rows x leading dimension in bytes below 4 GiB, for A and for B
    (G, gemm(M=1 << 22, K=1024), "4 GiB"), (G, gemm(Nn=1 << 22, K=1024), "4 GiB"), (G, gemm(M=1 << 21, K=1024, lda=2048), "4 GiB"),
    ("vtp_quantize_e4m3", quant(src=N), "bad argument"), ("vtp_quantize_e4m3", quant(dst=N), "bad argument"),
    ("vtp_quantize_e4m3", quant(n=12), "% 8"), ("vtp_quantize_e4m3", quant(n=0), "% 8"),
    ("vtp_amax", amax(src=N), "bad argument"), ("vtp_amax", amax(out=N), "bad argument"), ("vtp_amax", amax(n=12), "% 8"),
    ("vtp_amax", amax(n=0), "% 8"),
    ("vtp_dequantize_e4m3", dequant(src=N), "bad argument"), ("vtp_dequantize_e4m3", dequant(dst=N), "bad argument"),
    ("vtp_dequantize_e4m3", dequant(n=6), "% 4"), ("vtp_dequantize_e4m3", dequant(n=0), "% 4"),
]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    return _lib.load()


def test_every_fp8_entry_has_a_null_and_a_shape_case():
    names = {c[0] for c in CASES}
    assert names == {"vtp_gemm_nt_fp8", "vtp_quantize_e4m3", "vtp_amax", "vtp_dequantize_e4m3"}
    for name in names:
        tokens = [c[2] for c in CASES if c[0] == name]
        assert any(t in ("null", "bad argument") for t in tokens) and any(t not in ("null", "bad argument") for t in tokens), name


@pytest.mark.parametrize("name,args,token", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_refused_before_any_hip_call(lib, name, args, token):
    rc = getattr(lib, name)(*args)
    msg = lib.vtp_last_error().decode()
    assert rc == -1, f"{name}: rc {rc}"
    assert msg.startswith(name + ":"), msg
    assert token in msg, msg


def test_the_largest_operand_below_4_gib_is_not_refused_for_its_size(lib):
    """M x lda one row short of 4 GiB passes the staging check: with a null bias on the SwiGLU epilogue the refusal is that one"""
    rc = lib.vtp_gemm_nt_fp8(*gemm(M=(1 << 22) - 1, K=1024, epi=SWIGLU, bias=N))
    msg = lib.vtp_last_error().decode()
    assert rc == -1 and "SwiGLU" in msg and "4 GiB" not in msg, msg
