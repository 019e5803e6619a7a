"""The MFMA extend attention over MXFP4 caches without a GPU: the workspace rule of the two MXFP4 extend entries is unchanged — one partial per
SETOK_EXTEND_CHUNK slots, B * Tn * H * ceil((len0 + Tn) / 256) * (Dh + 2) floats whatever the element type — although the MFMA path (16 bits,
head dim 128) leaves fewer partials, one per span of up to four chunks, and uses a prefix of it.  Both builds and the Python helpers agree."""
import itertools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 256


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    from setok_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH) or not os.path.isfile(_lib.LIB_PATH_F16):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


# (len0, Tn): one chunk, its edges, and sums where a 1024-slot span of the MFMA path holds two, four and (in its second span) one and four chunks
SLOTS = [(0, 1), (0, 5), (255, 1), (256, 1), (248, 17), (253, 4), (1000, 7), (1020, 4), (1023, 2), (1030, 5), (300, 130), (512, 512), (2040, 8), (4000, 96)]


@pytest.mark.parametrize("half", [False, True])
def test_the_mxfp4_extend_workspaces_stay_one_partial_per_chunk(lib, half):
    sys.path.insert(0, ROOT)
    from setok_amd import ops
    import re
    header = open(os.path.join(ROOT, "include", "setok_hip.h")).read()
    assert int(re.search(r"#define\s+SETOK_EXTEND_CHUNK\s+(\d+)", header).group(1)) == CHUNK == ops.EXTEND_CHUNK
    assert int(re.search(r"#define\s+SETOK_ABI_VERSION\s+(\d+)", header).group(1)) == 9
    l = lib.load(half)
    assert l.setok_abi_version() == 9
    for (len0, Tn), B, H, Dh in itertools.product(SLOTS, (1, 3), (2, 8, 32), (32, 96, 128)):
        want = B * Tn * H * ((len0 + Tn + CHUNK - 1) // CHUNK) * (Dh + 2)
        assert l.setok_attention_extend_mxfp4kv_workspace(B, Tn, H, Dh, len0) == want, (B, Tn, H, Dh, len0)
        assert l.setok_attention_extend_paged_mxfp4kv_workspace(B, Tn, H, Dh, len0) == want, (B, Tn, H, Dh, len0)
        assert ops.attention_extend_mxfp4kv_workspace(B, Tn, H, Dh, len0) == want
        assert ops.attention_extend_paged_mxfp4kv_workspace(B, Tn, H, Dh, len0) == want
        # what the MFMA path writes — the native rule at the same shape — is a prefix of it
        code = 2 if half else 1
        for Hkv in (1, H):
            assert l.setok_attention_extend_workspace(code, B, Tn, H, Hkv, Dh, len0) <= want
    assert l.setok_attention_extend_mxfp4kv_workspace(1, 0, 8, 128, 5) == 0 and l.setok_attention_extend_mxfp4kv_workspace(1, 1, 8, 128, -1) == 0


@pytest.mark.parametrize("half", [False, True])
def test_the_mfma_grid_is_checked_on_the_host(lib, half):
    """16 bits at head dim 128 only: Hkv * ceil(G * Tn / 128) <= 65535, refused with SETOK_EINVAL before the workspace is looked at; fp32 and other head
    dims keep the wave-per-chunk grid and pass this check."""
    l = lib.load(half)
    dt = 2 if half else 1
    P = 4096                                                                   # stands in for device pointers: nothing is dereferenced
    H = Hkv = 512
    Tn = 128 * 128 + 1

    def dense(dtype=dt, Dh=128, Tn=Tn):
        return (None, dtype, P, H * Dh, P, P, P, P, P, P, 1, Tn, H, Hkv, Dh, Tn, 0, 0.1, P, 16)

    def paged(dtype=dt, Dh=128, Tn=Tn):
        return (None, dtype, P, H * Dh, P, P, P, P, P, 1 + Tn // 128, 4, P, P, 1, Tn, H, Hkv, Dh, 0, 0.1, P, 16)

    for fn, args, name in ((l.setok_attention_extend_gqa_mxfp4kv, dense, b"setok_attention_extend_mxfp4kv"),
                           (l.setok_attention_extend_gqa_paged_mxfp4kv, paged, b"setok_attention_extend_paged_mxfp4kv")):
        assert fn(*args()) == -1 and b"launch grid" in l.setok_last_error() and name in l.setok_last_error(), l.setok_last_error()
        for kw in (dict(Tn=127 * 128), dict(dtype=0), dict(Dh=64)):           # 512 * 127 blocks; fp32; another head dim: on to the workspace check
            assert fn(*args(**kw)) == -1 and b"workspace of" in l.setok_last_error(), (kw, l.setok_last_error())
