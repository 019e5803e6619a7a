"""The dispatch rules of the GEMM entry points, restated for the tests (gemm.hip: bf16_kernel; gemm_persist.hip: tail_shape_for, pp_takes, the peel of
setok_gemm_persist_bf16), and the K-tile widths read from the sources.  test_linear_abi_gpu.py and test_gemm_programs_gpu.py name a kernel class per case
and assert through `_kernel_class` that the case's shape reaches it on the device it runs on.  Needs no GPU except `_ncu`."""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "setok_amd", "csrc")


def source_constant(file, name):
    """The value of `constexpr int ... name = <integer>` in a file of setok_amd/csrc."""
    with open(os.path.join(CSRC, file)) as f:
        text = f.read()
    m = re.search(r"constexpr int [^;]*\b%s = (\d+)" % name, text)
    assert m, f"{file} has no constexpr int {name}"
    return int(m.group(1))


def _cdiv(a, b):
    return (a + b - 1) // b


def _ncu():
    from setok_amd import _lib
    return _lib.device_info()[1]


def _tail_shape(M, N, ncu, whole):
    t64 = _cdiv(M, 64) * _cdiv(N, 64)
    if whole and N % 64 == 0 and t64 > ncu:
        main, rem = (M // 128) * (N // 64), M % 128
        if ncu // 2 < main <= ncu and (rem == 0 or _cdiv(rem, 32) * (N // 32) <= main):
            return (128, 64, 6)
    if t64 * 4 <= ncu and N % 32 == 0:
        return (32, 32, 8)
    if N % 32 == 0 and _cdiv(M, 32) * _cdiv(N, 32) <= 2 * ncu:
        return (32, 32, 8)
    if t64 * 2 <= ncu and N % 32 == 0:
        return (64, 32, 8)                      # (unreachable: see test_linear_abi_gpu.py's docstring)
    if ncu < t64 <= 2 * ncu:
        return (64, 64, 4)
    return (64, 64, 8)


def _persist_class(M, N, K, ncu):
    tilesM, tilesN = _cdiv(M, 256), _cdiv(N, 256)
    T = tilesM * tilesN
    r, p = T % ncu, 0
    if T > ncu and r != 0 and r % tilesN == 0 and r // tilesN <= 2:
        p = r // tilesN
    if p == 0 and M % 256 != 0 and tilesM > 1 and N % 256 == 0:
        p = 1
    tm = tilesM - p
    main_rows = min(tm * 256, M)
    name = "pp" if (N % 256 == 0 and K >= 128 and main_rows % 256 == 0) else "persist"
    if p == 0:
        return name
    rem = M - tm * 256
    if name == "pp":
        sh = _tail_shape(rem, N, ncu, False)
        grid = min(tm * tilesN, ncu)
        shape = sh[0] if sh[0] == sh[1] and sh[2] == 8 else 64
        if _cdiv(rem, shape) * (N // shape) > grid:
            shape = 64
        if _cdiv(rem, shape) * (N // shape) <= grid:
            return "pp+rem"                     # the remainder rows inside the ping-pong launch
    return name + "+tail"                       # ... as a small-tile launch of their own


def _kernel_class(M, N, K, ldc, ncu, out16=True, batch=1, ln=False, plain=False):
    """The kernel a 16-bit-input problem goes to.  `plain`: no bias / activation / residual (what the fp32-out batched persistent kernel needs)."""
    tiles = _cdiv(M, 256) * _cdiv(N, 256)
    if out16 and batch == 1 and N % 64 == 0 and ldc % 8 == 0:
        if K >= 192 and tiles >= 90:
            return _persist_class(M, N, K, ncu)
        return "small %dx%d/%d" % _tail_shape(M, N, ncu, not ln)
    if not out16 and plain and N % 64 == 0 and K >= 192 and ldc % 4 == 0 and tiles * batch >= 96:
        return "f32b"
    return "tile128"


def _rows_reaching(want, M, N, K, ncu, ln=False):
    """`M` reaches class `want` on 256 CUs; on a device with another CU count: the first row count the rules send there."""
    if _kernel_class(M, N, K, N, ncu, ln=ln) == want:
        return M
    for m in range(1, 1 << 15):
        if _kernel_class(m, N, K, N, ncu, ln=ln) == want:
            return m
    pytest.fail(f"no row count reaches {want} at N={N} K={K} on {ncu} CUs")
