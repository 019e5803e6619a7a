"""The SeTok head's ragged attention (2 heads x 512), its backward, the cluster sort and the segment mean at the segment counts and mixes
the cluster encoders really run: thousands of segments (attn_seg_big_kernel<64> past 2048 of them), the encode form with an empty tail of
segments up to n_segs = rows, the inter-encoder form with rows that belong to no segment, and long segments whose softmax matters (logit sd
about 3, a dominant key planted in the first / the last / a one-key tail tile, a segment of all-zero queries).

Every reference is plain fp64 torch on the inputs rounded to the kernel's type: softmax(scale q k^T) v per segment, its autograd for the
backward; segments of equal length are stacked into one batch.  Errors are read per class of segment (length 1, 2-32, > 32) and for every
long segment alone: a long segment's output averages many rows of v and is about sqrt(n) times smaller than a short one's, so one bound
over all of them cannot see an error confined to the long ones.  `pytest -m gpu`."""
import functools
import os

import numpy as np
import pytest
import torch

import parity

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import _lib, ops

DEV = "cuda"
H, DH = 2, 512
C = H * DH
SCALE = DH ** -0.5
SIGMA_QK = 1.7                      # logit sd = SIGMA_QK^2 = 2.9: the softmax is far from uniform
LONG = (33, 64, 65, 255, 256, 257, 576, 1024)
PLANT = {1024: 1000, 257: 256, 576: 5}     # segment length -> key whose logit leads (the last tile, a one-key tail tile, the first tile)
ZERO_Q = 256                        # the segment whose queries are all zero: its softmax is exactly uniform
N_P1 = 33 * 64 + 1                  # > 2048 segments: attn_seg_big_kernel<64>, the last group of 64 holds one segment
DTYPES = (torch.bfloat16, torch.float16, torch.float32)

# bounds: about 3 x the worst reading measured on an MI355X (parity.close's three readings; bf16 / fp16: the MFMA kernels, fp32: the generic ones)
FWD_TOL = {torch.bfloat16: 1e-2, torch.float16: 1.2e-3, torch.float32: 1.5e-5}
BWD_TOL = {torch.bfloat16: 5e-2, torch.float16: 6e-3, torch.float32: 2e-5}
ABS_TOL = {torch.bfloat16: 1e-3, torch.float16: 1e-3, torch.float32: 3e-4}    # dq, dk behind a planted key (see the backward test)
MEAN_TOL = {torch.bfloat16: 8e-3, torch.float16: 1e-3, torch.float32: 5e-7}


# ---------------------------------------------------------------------------------------------------------------------------------------
# segment populations
# ---------------------------------------------------------------------------------------------------------------------------------------
class Pop:
    """A ragged batch: `lens[s]` rows per segment, `keys[s]` names its content (a seeded long / ladder segment, or None: filler rows);
    `rows` >= sum(lens) (the rows past the last segment belong to none); offsets has n_segs + 1 entries."""

    def __init__(self, lens, keys, rows=None, n_segs=None):
        self.lens, self.keys = list(lens), list(keys)
        total = sum(self.lens)
        self.rows = total if rows is None else rows
        self.n_segs = len(self.lens) if n_segs is None else n_segs
        offs = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.offs = np.concatenate([offs, np.full(self.n_segs - len(self.lens), total)]).tolist()      # empty tail: offsets = sum(lens)
        self.max_len = max(self.lens)
        self.covered = torch.zeros(self.rows, dtype=torch.bool)
        self.covered[:total] = True

    def segs(self, pred=lambda n: True):
        return [s for s, n in enumerate(self.lens) if n and pred(n)]

    def rows_of(self, segs):
        return torch.cat([torch.arange(self.offs[s], self.offs[s] + self.lens[s]) for s in segs])

    def where(self, n):
        """index of the (first) segment of length n"""
        return self.lens.index(n)


def _ladder():
    return list(range(1, 34)), [("ladder", n) for n in range(1, 34)]          # every length 1-33 once, 32 next to 33


@functools.lru_cache(maxsize=None)
def population(name):
    rng = np.random.default_rng(2024)
    if name in ("P1", "P1e"):
        lens = rng.integers(1, 9, N_P1).tolist()                                 # mostly 1-8 rows: the inner encoder's clusters
        keys = [None] * N_P1
        at = {0: 1024, 63: 65,                                                   # lanes 0 and 63 of the first group of 64
              64 + 20: 255, 64 + 21: 256, 64 + 22: 257,                           # three consecutive long ones in the second group
              64 * 17 + 30: 576,                                                 # alone in a middle group
              N_P1 - 1: 64}                                                      # the very last segment, alone in the last group
        for s, n in at.items():
            lens[s], keys[s] = n, ("long", n)
        ll, lk = _ladder()
        lens[200:233], keys[200:233] = ll, lk                                    # (33: the one long segment of the fourth group)
        assert sorted(n for n in lens if n > 32) == sorted(LONG)
        if name == "P1":
            return Pop(lens, keys)
        rows = sum(lens)
        return Pop(lens, keys, rows=rows, n_segs=rows)                           # the encode form: n_segs = rows, tail offsets = rows
    if name == "P2":                                                             # <= 2048 segments: attn_seg_big_kernel<1>
        fill = rng.integers(1, 9, 160).tolist()
        ll, lk = _ladder()
        lens, keys = fill[:40] + ll + fill[40:], [None] * 40 + lk + [None] * 120
        for i, n in enumerate(LONG[1:]):                                         # (33 is in the ladder)
            lens.insert(20 * i + 3, n); keys.insert(20 * i + 3, ("long", n))
        return Pop(lens, keys)
    if name == "P3":                                                             # the inter encoder: rows = B N, B segments, offsets[B] < rows
        lens = [1, 32, 33, 200, 576]
        keys = [("ladder", 1), ("ladder", 32), ("ladder", 33), ("long", 200), ("long", 576)]
        return Pop(lens, keys, rows=len(lens) * 576)
    raise KeyError(name)


def alone(n, kind="long"):
    return Pop([n], [(kind, n)])


def _content(key, n):
    """(n, 4C) fp32 rows q | k | v | dout of a named segment, the same in every population it appears in"""
    kind, length = key
    seed = {"long": 10_000, "ladder": 20_000}[kind] + length
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 4 * C, generator=g)
    x[:, :2 * C] *= SIGMA_QK
    if kind == "long" and length in PLANT:                   # one key whose logit leads every query's others by >= 8 (checked in `_attn_ref`)
        j = PLANT[length]
        for h in range(H):
            d0 = h * DH + 7
            x[:, d0] = 8.0                                    # every query: 8 along dim d0 ...
            x[j, C + h * DH:C + (h + 1) * DH] = 0.0
            x[j, C + d0] = 80.0                               # ... the planted key only along d0: logit scale * 8 * 80 = 28.3
    if kind == "long" and length == ZERO_Q:
        x[:, :C] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def _master(name):
    """(rows, 4C) fp32 content of a population (q | k | v | dout)"""
    p = population(name) if isinstance(name, str) else alone(*name)
    g = torch.Generator().manual_seed({"P1": 1, "P1e": 1, "P2": 2, "P3": 3}.get(name, 0) if isinstance(name, str) else 0)
    x = torch.randn(p.rows, 4 * C, generator=g)
    x[:, :2 * C] *= SIGMA_QK
    for s, n in enumerate(p.lens):
        if p.keys[s] is not None:
            x[p.offs[s]:p.offs[s] + n] = _content(p.keys[s], n)
    return x


def _pop(name):
    return population(name) if isinstance(name, str) else alone(*name)


@functools.lru_cache(maxsize=8)
def inputs(name, dt):
    """qkv and dout in the kernel's type, and the fp64 forward reference computed on them"""
    x = _master(name).to(dt)
    qkv, dout = x[:, :3 * C].contiguous(), x[:, 3 * C:].contiguous()
    return qkv, dout, _attn_ref(qkv, _pop(name))


def _groups(p):
    by_len = {}
    for s in p.segs():
        by_len.setdefault(p.lens[s], []).append(p.offs[s])
    for n, starts in by_len.items():
        yield n, torch.tensor(starts)[:, None] + torch.arange(n)                # (segments, n) row indices


def _attn(blk, n):
    """fp64 softmax(scale q k^T) v of a stack of equal-length segments: blk (G, n, 3C) -> (G, n, C)"""
    q, k, v = blk.reshape(blk.shape[0], n, 3, H, DH).permute(2, 0, 3, 1, 4)      # (G, H, n, DH) each
    a = torch.softmax(q @ k.transpose(-1, -2) * SCALE, -1)
    return (a @ v).transpose(1, 2).reshape(blk.shape[0], n, C)


def _attn_ref(qkv, p):
    x = qkv.double()
    out = torch.zeros(p.rows, C, dtype=torch.float64)
    for n, idx in _groups(p):
        out[idx] = _attn(x[idx], n)
    # the planted keys really lead: every query's logit for the planted key exceeds its others by >= 8
    for s in p.segs(lambda n: n in PLANT):
        n = p.lens[s]
        blk = x[p.offs[s]:p.offs[s] + n].reshape(n, 3, H, DH)
        lg = torch.einsum("ihd,jhd->hij", blk[:, 0], blk[:, 1]) * SCALE
        j = PLANT[n]
        others = torch.cat([lg[..., :j], lg[..., j + 1:]], -1).amax(-1)
        assert float((lg[..., j] - others).min()) >= 8.0, (n, float((lg[..., j] - others).min()))
    return out


def _attn_bwd_ref(qkv, dout, p):
    x, g = qkv.double(), dout.double()
    grad = torch.zeros_like(x)
    with torch.enable_grad():
        for n, idx in _groups(p):
            blk = x[idx].requires_grad_(True)
            _attn(blk, n).backward(g[idx])
            grad[idx] = blk.grad
    return grad


# ---------------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------------
_SENT = {torch.bfloat16: (torch.int16, 0x7FAB), torch.float16: (torch.int16, 0x7FAB), torch.float32: (torch.int32, 0x7FABCDEF)}  # NaN bits


def _sentinel(shape, dt):
    it, bits = _SENT[dt]
    t = torch.empty(shape, dtype=dt, device=DEV)
    t.view(it).fill_(bits)
    return t


def _holds_sentinel(t, dt):
    it, bits = _SENT[dt]
    return bool((t.view(it) == bits).all())


def _offsets(p):
    return torch.tensor(p.offs, dtype=torch.int32, device=DEV)


def _fwd(name, dt):
    p = _pop(name)
    qkv = inputs(name, dt)[0]
    out = _sentinel((p.rows, C), dt)
    ops.attention(qkv.to(DEV), H, DH, SCALE, seg_len=p.max_len, seg_offsets=_offsets(p), n_segs=p.n_segs, out=out)
    return out.cpu()


def _bwd(name, dt, out):
    p = _pop(name)
    qkv, dout, _ = inputs(name, dt)
    return ops.attention_bwd(qkv.to(DEV), out.to(DEV), dout.to(DEV), H, DH, SCALE, p.max_len, _offsets(p), p.n_segs).cpu()


CLASSES = (("len1", lambda n: n == 1), ("len2-32", lambda n: 2 <= n <= 32), ("len>32", lambda n: n > 32))


def _log(what, value, bound):
    log = os.environ.get("SETOK_PARITY_LOG")
    if log:
        test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        with open(log, "a") as f:
            f.write(f"{test}\t{what}\tmax_abs {value:.3e}\tbound {bound:.1e}\n")


def _check_classes(p, got, ref, tol, what, absolute=(), abs_tol=None):
    """parity.close per class of segment and per long segment, over the rows that belong to a segment.  Segments in `absolute`, and any
    whose reference is exactly zero (dq, dk of a one-row segment; dk of the all-zero-query segment), are held to an absolute bound instead:
    max |err| <= abs_tol x the rms of the reference over the other long segments."""
    rel = [s for s in range(len(p.lens)) if s not in absolute]
    parts = [(name, [s for s in p.segs(pred) if s in rel]) for name, pred in CLASSES]
    parts += [(f"seg{s}(n={p.lens[s]})", [s]) for s in p.segs(lambda n: n > 32)]
    floor = ref[p.rows_of([s for s in p.segs(lambda n: n > 32) if s in rel])].double().pow(2).mean().sqrt()
    for name, segs in parts:
        if not segs:
            continue
        r = p.rows_of(segs)
        g, e = got[r], ref[r]
        if segs[0] in absolute or float(e.abs().max()) == 0.0:
            bound = abs_tol * float(floor)
            m = float((g.double() - e.double()).abs().max())
            _log(f"{what} {name} (absolute)", m, bound)
            assert m <= bound, (what, name, m, bound)
        else:
            parity.close(g, e, tol, f"{what} {name}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. forward
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", ["P1", "P1e", "P2", "P3"])
def test_attention_segments_forward(name, dt):
    p = _pop(name)
    ref = inputs(name, dt)[2]
    got = _fwd(name, dt)
    cov = p.covered
    assert _holds_sentinel(got[~cov], dt), "rows that belong to no segment were written"
    assert not torch.isnan(got[cov]).any(), "a row of a segment was not written"
    _check_classes(p, got, ref, FWD_TOL[dt], f"out {name}")
    again = _fwd(name, dt)
    assert torch.equal(got.view(_SENT[dt][0]), again.view(_SENT[dt][0])), "two runs differ"


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16", "fp32"])
def test_attention_segment_bits_do_not_depend_on_the_launch(dt):
    """A segment's output bits are the same in P1 (> 2048 segments: big<64>), P2 (big<1>), P3 and launched alone: the same arithmetic in
    attn_seg_big_kernel<64> and <1>; the same for short segments (the small kernel)."""
    outs = {name: _fwd(name, dt) for name in ("P1", "P2", "P3")}
    for n, kind in [(n, "long") for n in LONG if n != 33] + [(n, "ladder") for n in (1, 7, 32, 33)]:
        solo = _fwd((n, kind), dt)
        for name, out in outs.items():
            p = _pop(name)
            hits = [s for s in p.segs() if p.keys[s] == (kind, n)]
            for s in hits:
                seg = out[p.offs[s]:p.offs[s] + n]
                assert torch.equal(seg.view(_SENT[dt][0]), solo.view(_SENT[dt][0])), (name, kind, n)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. backward
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.grad
@pytest.mark.parametrize("name,dt", [("P1", torch.bfloat16), ("P1e", torch.bfloat16), ("P3", torch.bfloat16),
                                     ("P1", torch.float16), ("P1e", torch.float16), ("P3", torch.float16), ("P1", torch.float32)],
                         ids=["P1-bf16", "P1e-bf16", "P3-bf16", "P1-fp16", "P1e-fp16", "P3-fp16", "P1-fp32"])
def test_attention_segments_backward(name, dt):
    p = _pop(name)
    qkv, dout, _ = inputs(name, dt)
    out = _fwd(name, dt)
    got = _bwd(name, dt, out)
    ref = _attn_bwd_ref(qkv, dout, p)
    # Behind a planted key the softmax saturates: dq and dk are then differences of nearly equal terms (ds = p (dp - D), D = dO . out with
    # `out` rounded to the kernel's type), about e^-8 of the other segments' gradients in fp64 and rounding noise in any kernel.  They are held
    # to an absolute bound in the scale of the well-conditioned long segments; dv (= P^T dO) stays relative everywhere.
    planted = p.segs(lambda n: n in PLANT)
    for i, part in enumerate(("dq", "dk", "dv")):
        cols = slice(i * C, (i + 1) * C)
        _check_classes(p, got[:, cols], ref[:, cols], BWD_TOL[dt], f"{part} {name}", absolute=planted if part != "dv" else (),
                       abs_tol=ABS_TOL[dt])
    again = _bwd(name, dt, out)
    cov = p.covered
    it = _SENT[dt][0]
    assert torch.equal(got[cov].view(it), again[cov].view(it)), "two runs differ"
    if name == "P1":                                    # a long segment launched alone: the same bits
        for n in (65, 257, 1024):
            s = p.where(n)
            solo = _bwd((n, "long"), dt, out[p.offs[s]:p.offs[s] + n])
            assert torch.equal(got[p.offs[s]:p.offs[s] + n].view(it), solo.view(it)), n


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. sort and segment mean at real sizes
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [196, 256, 576, 1024])
@pytest.mark.parametrize("B", [1, 37, 256])
def test_cluster_sort_real_sizes(B, N):
    g = torch.Generator().manual_seed(B * 10_000 + N)
    counts = torch.randint(1, N + 1, (B,), generator=g)
    counts[0], counts[-1] = 1, N                                                # (B = 1: one cluster of all N tokens)
    idx = torch.stack([torch.cat([torch.arange(int(L)), torch.randint(0, int(L), (N - int(L),), generator=g)])[torch.randperm(N, generator=g)]
                       for L in counts])                                        # every cluster id below counts[b] is used
    perm = torch.full((B * N,), -7, dtype=torch.int32, device=DEV)
    seg = torch.full((B * N + 1,), -7, dtype=torch.int32, device=DEV)
    img = torch.full((B + 1,), -7, dtype=torch.int32, device=DEV)
    idx_d, counts_d = idx.to(DEV), counts.int().to(DEV)
    _lib.call("setok_cluster_sort", ops._stream(), idx_d.data_ptr(), counts_d.data_ptr(), B, N, perm.data_ptr(), seg.data_ptr(), img.data_ptr())
    exp_perm, exp_seg = [], []
    for b in range(B):
        exp_perm.append(torch.sort(idx[b], stable=True).indices + b * N)
        sizes = torch.bincount(idx[b], minlength=int(counts[b]))
        exp_seg.append(b * N + torch.cumsum(sizes, 0) - sizes)
    total = int(counts.sum())
    exp_seg.append(torch.full((B * N + 1 - total,), B * N))                     # the empty tail up to B N
    assert torch.equal(img.cpu().long(), torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(counts, 0)]))
    assert torch.equal(perm.cpu().long(), torch.cat(exp_perm))
    assert torch.equal(seg.cpu().long(), torch.cat(exp_seg))


def _mean_inputs(name, dt):
    p = population(name)
    h = _master(name)[:, :C].to(dt)
    n_dev = torch.tensor([len(p.lens)], dtype=torch.int32, device=DEV)        # the number of real segments (< the launch bound in P1e)
    return p, h, n_dev


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", ["P1", "P1e"])
def test_segment_mean_real_counts(name, dt):
    p, h, n_dev = _mean_inputs(name, dt)
    out = _sentinel((p.n_segs, C), dt)
    ops.segment_mean(h.to(DEV), _offsets(p), n_dev, p.n_segs, out=out)
    out = out.cpu()
    real = len(p.lens)
    assert _holds_sentinel(out[real:], dt), "rows at or beyond n_segs_dev were written"
    ref = torch.stack([h[p.offs[s]:p.offs[s] + n].double().mean(0) for s, n in enumerate(p.lens)])
    got = out[:real]
    for cname, pred in CLASSES:
        segs = torch.tensor([s for s, n in enumerate(p.lens) if pred(n)])
        parity.close(got[segs], ref[segs], MEAN_TOL[dt], f"mean {name} {cname}")


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", ["P1", "P1e"])
def test_segment_mean_bwd_real_counts(name, dt):
    p, _, n_dev = _mean_inputs(name, dt)
    real = len(p.lens)
    dseg = torch.randn(p.n_segs, C, generator=torch.Generator().manual_seed(5)).to(dt)
    if p.n_segs > real:
        dseg[real:] = float("nan")                                             # past n_segs_dev: never read
    got = ops.segment_mean_bwd(dseg.to(DEV), _offsets(p), n_dev, p.n_segs, p.rows).cpu()
    lens = torch.tensor(p.lens)
    exact = (dseg[:real].float() / lens[:, None].float()).to(dt).repeat_interleave(lens, 0)
    assert torch.equal(got.view(_SENT[dt][0]), exact.view(_SENT[dt][0]))
    parity.close(got, (dseg[:real].double() / lens[:, None]).repeat_interleave(lens, 0), MEAN_TOL[dt], f"mean_bwd {name}")
