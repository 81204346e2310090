"""The exact fast paths of csrc/pt_exact.h on a real MI355X (include/ptc_exact_debug.h: ptc_debug_exact_arith).

The hook evaluates a fast path (guard + v_rcp_f32 / v_rsq_f32 seed + fma chain, or the compiler's expansion behind the guard's branch) and the compiler's correctly
rounded / or sqrtf on the device, under the library's own flags, and counts the operands whose bits differ.  Zero are allowed.

1. Reciprocal, square root and the two-rounding 1 / sqrt (root and reciprocal both compared): all 2^32 bit patterns each.
2. Division: 2^28 seeded pairs (every other pair with both exponents inside the guard's window, which uniform patterns hit once in sixteen), and the full cross
   product of a 4,096-value special set: zeros, denormals, powers of two at the guard's edges and their neighbours, infinities, NaNs, all-ones mantissas.
3. pt_div3 (three numerators over a divisor in [2^-5, 1], one of them +0 for a quarter of the operands): 2^28 seeded operands and the special set's cross product.
4. What the hook refuses."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RCP, SQRT, RNORM, DIV, DIV3 = range(5)
E_ARG = -1
_cache = {}


def _pt(pbr):
    if "pt" not in _cache:
        _cache["pt"] = pbr.PathTracer(0)
    return _cache["pt"]


def _show(off):
    f = off.view(np.float32)
    return "; ".join(f"a {f[k, 0]!r} ({off[k, 0]:08x}) b {f[k, 1]!r} ({off[k, 1]:08x}): fast {off[k, 2]:08x}, compiler {off[k, 3]:08x}" for k in range(len(off)))


def special_set():
    """4,096 float32 values: the operands a guard, an expansion or a chain could mishandle, then seeded patterns of the whole range and of the guard's window."""
    u = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00400000, 0x00800000, 0x80800000, 0x00800001, 0x00ffffff,
         0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0x7f7fffff, 0xff7fffff, 0x7f000000, 0x3f800000, 0xbf800000,
         0x3f800001, 0x3f7fffff, 0x3fffffff, 0x40000000, 0x3effffff, 0x3d4ccccd, 0x3d000000, 0x3cffffff]      # ..., 0.05, 2^-5 and the pattern below it
    for e in (1, 2, 30, 31, 32, 33, 34, 62, 63, 64, 65, 94, 95, 96, 97, 126, 127, 128, 157, 158, 159, 160, 190, 191, 192, 222, 223, 224, 253, 254):   # window: [95, 159)
        for m in (0x000000, 0x000001, 0x7ffffc, 0x7ffffd, 0x7ffffe, 0x7fffff, 0x400000, 0x3504f3):
            u += [(e << 23) | m, 0x80000000 | (e << 23) | m]
    u = np.array(u, np.uint32)
    rng = np.random.default_rng(20260131)
    rest = 4096 - len(u)
    wide = rng.integers(0, 1 << 32, rest // 2, dtype=np.uint64).astype(np.uint32)
    r = rng.integers(0, 1 << 32, rest - rest // 2, dtype=np.uint64).astype(np.uint32)
    window = (r & np.uint32(0x807fffff)) | ((np.uint32(95) + ((r >> np.uint32(23)) & np.uint32(63))) << np.uint32(23))
    s = np.concatenate([u, wide, window])
    assert s.shape == (4096,)
    return s.view(np.float32)


@pytest.mark.parametrize("op,name", [(RCP, "pt_rcp"), (SQRT, "pt_sqrt"), (RNORM, "pt_rnorm")])
def test_every_bit_pattern_gets_the_compilers_bits(pbr, op, name):
    bad, off = _pt(pbr).exact_arith(op, n=1 << 32, first=0)
    print(f"{name}: {bad} of 2^32 patterns differ")
    assert bad == 0, f"{name}: {bad} mismatches, first: {_show(off)}"


@pytest.mark.parametrize("op,name", [(DIV, "pt_div"), (DIV3, "pt_div3")])
def test_seeded_pairs_get_the_compilers_bits(pbr, op, name):
    bad, off = _pt(pbr).exact_arith(op, n=1 << 28, first=0x5eed0001)
    print(f"{name}: {bad} of 2^28 seeded pairs differ")
    assert bad == 0, f"{name}: {bad} mismatches, first: {_show(off)}"


@pytest.mark.parametrize("op,name", [(DIV, "pt_div"), (DIV3, "pt_div3")])
def test_cross_product_of_the_special_set_gets_the_compilers_bits(pbr, op, name):
    s = special_set()
    bad, off = _pt(pbr).exact_arith(op, s, s, cross=True)
    print(f"{name}: {bad} of 4096^2 special pairs differ")
    assert bad == 0, f"{name}: {bad} mismatches, first: {_show(off)}"


def test_one_operand_ops_on_the_special_set(pbr):
    """The explicit-operand mode of the one-operand ops, on values whose results are known on the host: numpy's float32 / and sqrt are IEEE too."""
    s = special_set()
    for op in (RCP, SQRT, RNORM):
        bad, off = _pt(pbr).exact_arith(op, s)
        assert bad == 0, (op, _show(off))


def test_what_the_hook_refuses(pbr):
    import ctypes as C

    pt = _pt(pbr)
    L, out = pbr.load_library(), (C.c_uint64 * 65)()
    a = (C.c_float * 4)(1.0, 2.0, 3.0, 4.0)
    assert L.ptc_debug_exact_arith(None, RCP, None, None, 4, 0, 0, out) == E_ARG
    for args in ((RCP, None, None, 4, 0, 0, None), (-1, None, None, 4, 0, 0, out), (5, None, None, 4, 0, 0, out), (RCP, None, None, 0, 0, 0, out),
                 (RCP, None, None, (1 << 32) + 1, 0, 0, out), (DIV, None, a, 4, 0, 0, out), (DIV, None, None, 4, 0, 1, out), (DIV, a, None, 4, 0, 1, out),
                 (RCP, a, a, 4, 0, 1, out), (DIV, a, a, (1 << 16) + 1, 0, 1, out), (RCP, a, None, (1 << 28) + 1, 0, 0, out)):
        assert L.ptc_debug_exact_arith(pt._h, *args) == E_ARG, args
