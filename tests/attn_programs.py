"""Score programs for the online-softmax attention kernels: inputs whose scaled scores follow a chosen profile over the keys, so that a kernel's
running-maximum branch is taken where — and as hard as — the test wants.  Pure torch on the CPU; imports nothing of the library.

`build` draws q, k ~ 0.5 randn and v ~ randn and steers through dimension 0: q[:, 0] = a_i and k[:, 0] = g_j.  With a_i = sqrt(Dh) and
scale = Dh ** -0.5 key j sits g_j nats above the rest on every steered row, over a noise of about a quarter nat from the other dims.  The caller
rounds q, k, v to the element type and computes every reference from the rounded tensors (sqrt(Dh) itself is rounded where Dh is no power of 4:
the offsets then scale by that factor on the kernel's side and on the reference's alike).

`walk` replays the tile walk of attn_vit_kernel (setok_amd/csrc/attn_vit.hip) in fp32 and counts what the inputs make it do; `emulate` is the same
walk producing an output, with the roundings of the 16-bit kernel: the bound a test asserts on the GPU is first shown attainable here.

`build_cache` is `build` for a (queries, cached keys) problem — the extend and decode kernels — and `emulate_chunked` the per-row replay of their
chunked walk (setok_amd/csrc/attn_extend.hip, attn_decode.hip, attn_partials.h): an online softmax over key tiles inside a span, one fp32 partial per
span, the merge of attn_decode_merge_kernel.  It also reports the smallest factors the inputs make the walk apply."""
import math
from typing import List, NamedTuple

import torch

DEFER_NATS = 8 * math.log(2.0)                     # attn_vit.hip: DEFER_MAX = 8 powers of two, in scaled-score units
LOG2E = 1.4426950408889634
SHORT_TAIL = 8                                     # a last key tile of at most this many keys runs the short form

STAIRS = {"stair4": 4.0, "stair5.5": 5.5, "stair8": 8.0, "down8": -8.0, "onerow8": 8.0}
PROGRAMS = ("stair4", "stair5.5", "stair8", "down8", "hot@0", "hot@31", "hot@32", "hot@lasttile", "hot@T-1", "shift-60", "onerow8")


def hot_key(program: str, T: int, tile: int = 32) -> int:
    """The key a `hot@...` program heats: a number, `T-1`, or `lasttile` (the first key of the last key tile)."""
    where = program.split("@", 1)[1]
    if where == "T-1":
        return T - 1
    if where == "lasttile":
        return (T - 1) // tile * tile
    return int(where)


def offsets(T: int, program: str, tile: int = 32) -> torch.Tensor:
    """g_j of the program: the offset of key j in nats, fp32."""
    j = torch.arange(T)
    if program in STAIRS:
        return STAIRS[program] * (j // tile).float()
    if program in ("shift-60", "shift-64"):        # -64 is the level an MXFP4 block carries exactly (-60 comes back as -48)
        return torch.full((T,), float(program[5:]))
    if program.startswith("hot@"):
        g = torch.zeros(T)
        p = hot_key(program, T, tile)
        if 0 <= p < T:                             # (a hot key past the end heats nothing: the caller plants it in memory the kernel must not read)
            g[p] = 16.0
        return g
    raise ValueError(f"unknown score program {program!r}")


def build(T: int, Dh: int, program: str, seed: int, Tq: int = None, tile: int = 32):
    """(q, k, v) of one head, fp32: q (Tq, Dh) — Tq = T unless given (cross-attention) —, k and v (T, Dh)."""
    Tq = T if Tq is None else Tq
    g = torch.Generator().manual_seed(seed)
    q = 0.5 * torch.randn(Tq, Dh, generator=g)
    k = 0.5 * torch.randn(T, Dh, generator=g)
    v = torch.randn(T, Dh, generator=g)
    a = torch.full((Tq,), math.sqrt(Dh))
    if program == "onerow8":
        a = torch.where(torch.arange(Tq) % 32 == 5, a, torch.zeros(Tq))
    q[:, 0] = a
    k[:, 0] = offsets(T, program, tile)
    return q, k, v


def reference(q, k, v, scale):
    """softmax(q k^T scale) v in fp64."""
    q, k, v = q.double(), k.double(), v.double()
    return torch.softmax(q @ k.t() * scale, -1) @ v


def errors(got, ref):
    """(global max-rel error, worst per-row max-rel error): max |err| / max |ref| over everything, and over the last dim of each row."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = (got - ref).abs()
    glob = float(err.max() / ref.abs().max().clamp_min(1e-30))
    rows = float((err.amax(-1) / ref.abs().amax(-1).clamp_min(1e-30)).max())
    return glob, rows


class Walk(NamedTuple):
    late: int                                      # rescales at a key tile > 0
    short_tail: int                                # of those, the ones the short form of the last tile took
    log2_pmax: float                               # log2 of the largest probability formed


def _walk_tile(s, n_valid, tile, defer_raw, c, on_tile=None):
    """One wave: s (32, T) raw fp32 scores of a query tile.  Yields the kernel's decisions; `on_tile(kt, lo, hi, m_run, alpha)` sees every step
    (alpha is None where the wave does not rescale)."""
    T = s.shape[1]
    nkv = (T + tile - 1) // tile
    m_run = torch.full((s.shape[0],), -math.inf)
    late = short = 0
    pmax = -math.inf
    for kt in range(nkv):
        lo, hi = kt * tile, min(T, (kt + 1) * tile)
        mx = s[:, lo:hi].amax(1)
        alpha = None
        if bool((mx > m_run + defer_raw).any()):                   # __any over the wave (rows past Tq repeat row Tq - 1: no new vote)
            m_new = torch.maximum(m_run, mx)
            alpha = torch.exp2((m_run - m_new) * c)
            m_run = m_new
            if kt > 0:
                late += 1
                short += int(kt == nkv - 1 and T % tile != 0 and T - lo <= SHORT_TAIL)
        pmax = max(pmax, float(((s[:n_valid, lo:hi] - m_run[:n_valid, None]) * c).max()))
        if on_tile is not None:
            on_tile(kt, lo, hi, m_run, alpha)
    return Walk(late, short, pmax)


def walk_qtiles(q, k, scale, tile: int = 32, defer_nats: float = DEFER_NATS) -> List[Walk]:
    """The walk of every query tile of 32 rows: one `Walk` per wave-sized unit."""
    q, k = q.float(), k.float()
    c = scale * LOG2E                                              # scale_log2e
    defer_raw = defer_nats / scale                                 # (float)DEFER_MAX / scale_log2e, in raw score units
    out = []
    for q0 in range(0, q.shape[0], 32):
        s = q[q0:q0 + 32] @ k.t()
        out.append(_walk_tile(s, s.shape[0], tile, defer_raw, c))
    return out


def walk(q, k, scale, tile: int = 32, defer_nats: float = DEFER_NATS) -> Walk:
    """fp32 replay of the deferred-maximum tile walk: (late rescales, short-tail rescales, log2 of the largest probability) over all query tiles."""
    w = walk_qtiles(q, k, scale, tile, defer_nats)
    return Walk(sum(x.late for x in w), sum(x.short_tail for x in w), max(x.log2_pmax for x in w))


def emulate(q, k, v, scale, dt, tile: int = 32, defer_nats: float = DEFER_NATS):
    """The same walk with the kernel's arithmetic: fp32 scores of the `dt` inputs, p = exp2(s c - m c) in fp32, the row sum over the UNROUNDED
    probabilities, P rounded to `dt` for the PV product (fp32 accumulation), the running rescale of sum and accumulators, the quotient rounded to `dt`."""
    q, k, v = q.to(dt).float(), k.to(dt).float(), v.to(dt).float()
    c = scale * LOG2E
    defer_raw = defer_nats / scale
    out = torch.empty(q.shape[0], v.shape[1], dtype=dt)
    for q0 in range(0, q.shape[0], 32):
        s = q[q0:q0 + 32] @ k.t()
        o = torch.zeros(s.shape[0], v.shape[1])
        l_run = torch.zeros(s.shape[0])

        def step(kt, lo, hi, m_run, alpha):
            nonlocal o, l_run
            if alpha is not None:
                l_run = l_run * alpha
                o = o * alpha[:, None]
            p = torch.exp2(s[:, lo:hi] * c - (m_run * c)[:, None])
            l_run = l_run + p.sum(1)
            o = o + p.to(dt).float() @ v[lo:hi]

        _walk_tile(s, s.shape[0], tile, defer_raw, c, step)
        out[q0:q0 + 32] = (o * (1.0 / l_run)[:, None]).to(dt)
    return out


# ---- cached keys: the extend and decode kernels -------------------------------------------------------------------------------------------------
NEG = -1.0e30                                      # attn_extend.hip's finite sentinel of a slot that does not count
LN2 = 0.69314718055994530942
FAULTS = ("no_rescale", "log2_max")                # planted errors of emulate_chunked (tests/test_cache_attn_programs_cpu.py); never in a kernel


def build_cache(Tq: int, n: int, Dh: int, G: int, program: str, seed: int, tile: int = 32):
    """(q (Tq, G, Dh), k (n, Dh), v (n, Dh)), fp32: one key / value head of a cache of n slots and the G query heads it serves, Tq query rows each.
    Steered through dimension 0 as `build` does: q[..., 0] = sqrt(Dh), k[:, 0] = offsets(n, program, tile)."""
    g = torch.Generator().manual_seed(seed)
    q = 0.5 * torch.randn(Tq, G, Dh, generator=g)
    k = 0.5 * torch.randn(n, Dh, generator=g)
    v = torch.randn(n, Dh, generator=g)
    q[..., 0] = math.sqrt(Dh)
    k[:, 0] = offsets(n, program, tile)
    return q, k, v


def _dec_exp(x, dt):
    """attn_partials.h's dec_exp: expf in fp32, v_exp_f32 of x log2(e) in the 16-bit types."""
    return torch.exp(x) if dt == torch.float32 else torch.exp2(x * LOG2E)


def emulate_chunked(q, k, v, counts, scale, dt, span: int, tile: int = 32, fault: str = None):
    """Per-row replay of the chunked walk with the kernel's roundings.  q (..., R, Dh), k and v (..., n, Dh), counts (..., R, n) bool: row r counts
    slot j.  fp32 scores of the `dt` inputs in log2 units; a slot that does not count is replaced by the -1e30 sentinel BY SELECTION (its K row may
    be NaN) and a V row that counts for no row is zeroed; the online maximum, sum and accumulators run over `tile`-key tiles inside each span of
    `span` slots; P is rounded to `dt` for the PV product, the sum is taken over the unrounded values; a span's partial is (m ln2, l, o), or
    (-inf, 0, 0) for a row that counted nothing in it; the merge runs in span order by the rule of attn_decode_merge_kernel.  tile = span is one
    softmax per chunk: the generic kernel, and a decode kernel's chunk when its wave slices are not modelled.
    Returns (out (..., R, Dh) in `dt`, the smallest rescale factor applied inside a span to a row that had counted a key, the smallest merge
    factor applied to a partial that had) — 1.0 where none was applied.  `fault` plants one error: "no_rescale" leaves the accumulators
    unscaled when the maximum moves, "log2_max" leaves the partial's maximum in log2 units."""
    assert fault is None or fault in FAULTS
    q, k, v = q.to(dt).float(), k.to(dt).float(), v.to(dt).float()
    n = k.shape[-2]
    t = torch.where(counts, (q @ k.transpose(-1, -2)) * (scale * LOG2E), torch.full((), NEG))
    v = torch.where(counts.any(-2)[..., None], v, torch.zeros(()))
    rows = t.shape[:-1]
    min_rescale = min_merge = 1.0
    parts = []
    for s0 in range(0, n, span):
        m_run, l_run, o = torch.full(rows, NEG), torch.zeros(rows), torch.zeros(rows + (v.shape[-1],))
        for k0 in range(s0, min(n, s0 + span), tile):
            tt = t[..., k0:k0 + tile]
            m_new = torch.maximum(m_run, tt.amax(-1))
            alpha = torch.exp2(m_run - m_new)
            moved = (m_run > NEG) & (m_new > m_run)
            if bool(moved.any()):
                min_rescale = min(min_rescale, float(alpha[moved].min()))
            l_run = l_run * alpha
            if fault != "no_rescale":
                o = o * alpha[..., None]
            m_run = m_new
            p = torch.where(tt <= NEG, torch.zeros(()), torch.exp2(tt - m_run[..., None]))
            l_run = l_run + p.sum(-1)
            o = o + p.to(dt).float() @ v[..., k0:k0 + tile, :]
        some = m_run > NEG
        mc = torch.where(some, m_run * (1.0 if fault == "log2_max" else LN2), torch.full((), -math.inf))
        parts.append((mc, torch.where(some, l_run, torch.zeros(())), torch.where(some[..., None], o, torch.zeros(()))))
    M = torch.stack([mc for mc, _, _ in parts]).amax(0)
    L, O = torch.zeros(rows), torch.zeros(rows + (v.shape[-1],))
    for mc, l, o in parts:
        some = mc > -math.inf
        f = torch.where(some, _dec_exp(mc - M, dt), torch.zeros(()))
        if bool(some.any()):
            min_merge = min(min_merge, float(f[some].min()))
        L = L + f * l
        O = O + f[..., None] * o
    inv = torch.where(L > 0, 1.0 / L, torch.zeros(()))
    return (O * inv[..., None]).to(dt), min_rescale, min_merge
