"""The paged attention kernels where their sentinel paths must matter: the score programs of tests/attn_programs.py through
setok_attention_decode_gqa_paged (attn_paged.hip) and setok_attention_extend_gqa_paged (attn_extend_paged.hip: the one-wave and four-wave MFMA
kernels and the generic twin).  Both files are copies of the dense kernels with the page lookup in the mask's place; tests/test_paged_gpu.py and
tests/test_prefix_gpu.py hold them to the dense kernels on `randn` data, where the only "no page" is the middle page of a 300-slot sequence.  Here
the stairs put e^-8 at every wave slice, key tile, page, chunk and span, a hot key sits 16 nats up on either side of each edge and in the slot just
past the end, and every launch runs under five tables: whole; the leading page(s) missing in front of live ones; a middle page missing; the page(s)
under the last slots — for extend, under the new rows — missing; every page missing.

A launch is ragged: sequences of different lengths, one empty / idle, `max_len` above the longest, the slots scattered over a pool at a random
permutation's pages.  Spare pages hold a finished sequence's data — finite K rows with the 16-nat hot value in k[:, 0] under NaN V —, a page a
table case takes away keeps its data in the pool, every slot at or above a sequence's end is NaN, and the slot a `hot@` program heats keeps, where it
lies past the end, its finite hot K row over a NaN V row.

Every (program, table) asserts: `torch.equal` to the dense kernel sequence by sequence (ops.attention_decode / ops.attention_extend at B = 1 on the
gathered slots under a mask that is zero exactly on the missing pages: page-aligned, so the same partition); finite outputs and the global and
worst per-row max-rel error against fp64 below the project's bound (`_tol` in 16 bits, `_bounds32` in fp32); equal bits on a second run and with
a NaN-poisoned workspace; exact zeros for the sequences without a live key.  Every figure goes to SETOK_PARITY_LOG
(profiles/mxfp4kv_paged_attn_programs_parity.txt).  `pytest -m gpu`."""
import pytest
import torch

import attn_programs as AP
import test_cache_attn_programs_gpu as G
from test_attn_programs_gpu import NAME, _Cases, _bounds32, _decode_ref32
from test_extend_gpu import _extend_ref, _tol
from test_generate_gpu import _decode_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import ops

DEV = "cuda"
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
NAN = float("nan")
PAGE = 128
SPARE = 3                                                              # pool pages no table names
TABLES = ("whole", "lead", "middle", "last", "none")


def missing_pages(table, P, new0):
    """The pages, of a sequence's P, that a table case takes away; `new0` is the page of the first of the last slots (decode: of the last slot;
    extend: of the first new row).  A case that would leave a sequence meant to keep keys without a page takes none of that sequence's."""
    if table == "none":
        return set(range(P))
    if table == "lead" and P >= 2:
        return set(range(max(1, P // 3)))
    if table == "middle" and P >= 3:
        return {P // 2}
    if table == "last" and new0 >= 1:
        return set(range(new0, P))
    return set()


class Problem:
    """One launch's pools and queries for a program.  ends[b]: slots of sequence b that hold keys (0: empty / idle); new0[b]: the first of its last
    slots; pages[b]: its pool pages in slot order; dense[b]: its slots as (Hkv, P * PAGE, Dh) K and V in `dt`, as the pool holds them."""

    def __init__(self, dt, Dh, H, Hkv, ends, new0, Tq, program, tile, seed):
        Gq, B = H // Hkv, len(ends)
        self.ends, self.new0, self.Tq = list(ends), list(new0), Tq
        self.P = [(e + PAGE - 1) // PAGE for e in ends]
        self.num_pages = sum(self.P) + SPARE
        g = torch.Generator().manual_seed(seed)
        perm = torch.randperm(self.num_pages, generator=g).tolist()
        self.pages = [[perm.pop() for _ in range(p)] for p in self.P]
        self.spare = perm
        hot = int(program[4:]) if program.startswith("hot@") else -1
        q = torch.empty(B, Tq, Hkv, Gq, Dh)
        kp = torch.full((self.num_pages, Hkv, PAGE, Dh), NAN)
        vp = kp.clone()
        self.dense = []
        for b, (e, p) in enumerate(zip(ends, self.P)):
            cap = p * PAGE
            k, v = torch.empty(Hkv, cap, Dh), torch.empty(Hkv, cap, Dh)
            for j in range(Hkv):
                q[b, :, j], kk, vv = AP.build_cache(Tq, max(cap, 1), Dh, Gq, program, seed + 100 * b + j, tile)
                k[j], v[j] = kk[:cap], vv[:cap]
            dead_k = torch.arange(cap) >= e
            if e <= hot < cap:
                dead_k[hot] = False                                    # past the end, in the sequence's last page: a finite hot K row over a NaN V row
            k[:, dead_k], v[:, e:] = NAN, NAN
            for i, page in enumerate(self.pages[b]):
                kp[page], vp[page] = k[:, i * PAGE:(i + 1) * PAGE], v[:, i * PAGE:(i + 1) * PAGE]
            self.dense.append((k.to(dt), v.to(dt)))
        for page in self.spare:                                        # a finished sequence's data: keys that would win, values that would show
            kp[page] = 0.5 * torch.randn(Hkv, PAGE, Dh, generator=g)
            kp[page][..., 0] = 16.0
        self.q, self.kp, self.vp = q.reshape(B * Tq, H * Dh).to(dt), kp.to(dt), vp.to(dt)

    def table(self, case):
        """(block table (B, max_pages) int32 — a missing page's entry is an id outside the pool —, masks[b] (P * PAGE,) uint8: 1 on the slots below the
        end that lie in a page the table names)."""
        bad = (-1, self.num_pages, 1 << 30)
        t = torch.full((len(self.ends), max(self.P) + 1), -1, dtype=torch.int32)
        masks = []
        for b, (e, p) in enumerate(zip(self.ends, self.P)):
            miss = missing_pages(case, p, self.new0[b] // PAGE)
            m = torch.zeros(p * PAGE, dtype=torch.uint8)
            m[:e] = 1
            for i, page in enumerate(self.pages[b]):
                t[b, i] = bad[(b + i) % 3] if i in miss else page
                if i in miss:
                    m[i * PAGE:(i + 1) * PAGE] = 0
            masks.append(m)
        return t, masks


def table_cases(P, new0):
    """The table cases of a launch, without those that take no page of any sequence (the middle page of two) and so are the whole case again."""
    return [c for c in TABLES if c == "whole" or any(missing_pages(c, p, n0 // PAGE) for p, n0 in zip(P, new0))]


def _check_launch(cases, name, dt, Dh, pb, case, paged, dense, ref64, ref32):
    """One (program, table): paged(table, ws) -> (B * Tq, H * Dh); dense(b, mask), ref64(b, mask), ref32(b, mask) -> sequence b's rows."""
    table, masks = pb.table(case)
    live = [bool(m.any()) for m in masks]
    rows, width = pb.Tq, pb.q.shape[1]
    ref = torch.cat([ref64(b, m) if ok else torch.zeros(rows, width, dtype=torch.float64) for b, (m, ok) in enumerate(zip(masks, live))])
    if dt != F32:
        bound = (_tol(dt, Dh),) * 2
    else:
        bound = _bounds32(torch.cat([ref32(b, m) if ok else torch.zeros(rows, width) for b, (m, ok) in enumerate(zip(masks, live))]), ref, Dh)
    table = table.to(DEV)
    got = paged(table, None)
    want = torch.cat([dense(b, m.to(DEV)) if ok else torch.zeros(rows, width, dtype=dt, device=DEV) for b, (m, ok) in enumerate(zip(masks, live))])
    cases.check(name, got, ref, Dh, *bound)
    cases.same_bits(name + " against the dense kernel", got, want)
    cases.same_bits(name + " second run", paged(table, None), got)
    cases.same_bits(name + " poisoned workspace", paged(table, NAN), got)
    for b, ok in enumerate(live):
        if not ok and G._not_zero(got.reshape(len(live), -1), b):
            cases.bad.append(f"{name}: sequence {b}, which has no live key, is not zero")
    return got


def _tables_mattered(cases, what, whole, gots):
    """Every table case changed the bits of the whole case under some program: the pages it takes away held keys that counted."""
    for case, outs in gots.items():
        if all(torch.equal(o, w) for o, w in zip(outs, whole)):
            cases.bad.append(f"{what} table={case}: no program's output differs from the whole table's")


# ---- decode --------------------------------------------------------------------------------------------------------------------------------------
# (dt, Dh, H, Hkv, n): 16 / 8 / 2 / 32 lanes per row and GT = 8 / 2 / 4 / 1 query heads per workgroup in 16 bits; 4 and 32 lanes, GT = 4 and 2 in fp32
DECODE_CASES = [(dt, Dh, H, Hkv, n) for dt in (BF, HF) for Dh, H, Hkv in ((128, 8, 1), (64, 4, 2), (16, 4, 1), (256, 2, 2)) for n in (129, 1000)]
DECODE_CASES += [(F32, Dh, H, Hkv, n) for Dh, H, Hkv in ((16, 4, 1), (128, 2, 1)) for n in (129, 1000)]


def decode_lens(n):
    """Five sequences: two of n slots, a shorter one, an empty one, one of about half."""
    return [n, n - 35, 0, n, n // 2 + 1]


def decode_programs(n):
    """n = 129: stairs at the wave's 32-key slice (the combine in LDS), a hot key on either side of a slice edge and of the page edge, and in slot n;
    n = 1000: stairs at the page (the merge; eight partials), a hot key on either side of the first page edge, in the last slot and in slot n."""
    if n == 129:
        return G._programs_with_hot([("stair8", 32), ("down8", 32)], [31, 32, 127, 128, 129])
    return G._programs_with_hot([("stair8", PAGE), ("down8", PAGE)], [127, 128, n - 1, n])


def decode_problem(dt, Dh, H, Hkv, n, program, tile):
    lens = decode_lens(n)
    return Problem(dt, Dh, H, Hkv, lens, [max(e - 1, 0) for e in lens], 1, program, tile, seed=800 + n)


def _decode_id(case):
    dt, Dh, H, Hkv, n = case
    return f"{NAME[dt]}-Dh{Dh}-H{H}-Hkv{Hkv}-len{n}"


@pytest.mark.parametrize("case", DECODE_CASES, ids=_decode_id)
def test_paged_decode_programs(case):
    dt, Dh, H, Hkv, n = case
    scale, cases = Dh ** -0.5, _Cases()
    lens = decode_lens(n)
    max_len = ((max(lens) + PAGE - 1) // PAGE) * PAGE + 100            # above the longest: every sequence has a trailing empty chunk
    dlens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    whole, gots = [], {}
    for program, tile in decode_programs(n):
        pb = decode_problem(dt, Dh, H, Hkv, n, program, tile)
        q, kp, vp = pb.q.to(DEV), pb.kp.to(DEV), pb.vp.to(DEV)
        dd = [(k[None, :, :e].contiguous().to(DEV), v[None, :, :e].contiguous().to(DEV)) for (k, v), e in zip(pb.dense, lens)]

        def paged(table, fill):
            ws = None if fill is None else torch.full((ops.attention_decode_paged_workspace(len(lens), H, Dh, max_len),), fill, device=DEV)
            return ops.attention_decode_paged(q, kp, vp, table, dlens, H, max_len, scale, ws=ws)

        def dense(b, m):
            return ops.attention_decode(q[b:b + 1], dd[b][0], dd[b][1], m[None, :lens[b]].contiguous(), H, lens[b], scale)

        def ref64(b, m):
            k, v = pb.dense[b]
            return _decode_ref(pb.q[b:b + 1], k[None], v[None], m[None], H, Hkv, Dh, lens[b])

        def ref32(b, m):
            k, v = pb.dense[b]
            return _decode_ref32(pb.q[b:b + 1], k[None], v[None], m[None], H, Hkv, Dh, lens[b])

        for case_t in table_cases(pb.P, pb.new0):
            name = f"paged decode {NAME[dt]} Dh={Dh} H={H} Hkv={Hkv} len={n} {G._label(program, tile)} table={case_t}"
            got = _check_launch(cases, name, dt, Dh, pb, case_t, paged, dense, ref64, ref32)
            (whole if case_t == "whole" else gots.setdefault(case_t, [])).append(got)
    _tables_mattered(cases, f"paged decode {_decode_id(case)}", whole, gots)
    cases.done()


# ---- extend --------------------------------------------------------------------------------------------------------------------------------------
# (dt, Dh, H, Hkv, Tn, len0).  Head dim 128 in 16 bits: exactly 32 stacked rows and 28 on the one-wave kernel; 136 rows on the four-wave kernel across
# the chunk edge and across the 1024-slot span edge; G = 1.  Everything else is the generic twin.
EXTEND_CASES = [(dt, 128) + rest for dt in (BF, HF) for rest in ((8, 1, 4, 253), (4, 2, 7, 300), (8, 1, 17, 248), (8, 1, 17, 1016), (2, 2, 40, 1000))]
EXTEND_CASES += [(dt, Dh, 4, 2, Tn, len0) for dt, Dh in ((F32, 16), (BF, 64), (HF, 32)) for Tn, len0 in ((17, 248), (7, 1000))]


def extend_len0s(len0):
    """Four sequences: len0 old slots, a shorter one, an idle one, another shorter one.  Every one that is not idle has a page below its new rows."""
    return [len0, len0 - 100, -1, len0 - 37]


def extend_problem(dt, Dh, H, Hkv, Tn, len0, program, tile):
    l0 = extend_len0s(len0)
    return Problem(dt, Dh, H, Hkv, [l + Tn if l >= 0 else 0 for l in l0], [max(l, 0) for l in l0], Tn, program, tile, seed=900 + len0 + Tn)


@pytest.mark.parametrize("case", EXTEND_CASES, ids=G._case_id)
def test_paged_extend_programs(case):
    dt, Dh, H, Hkv, Tn, len0 = case
    scale, cases = Dh ** -0.5, _Cases()
    l0 = extend_len0s(len0)
    max_len0 = ((len0 + Tn + PAGE - 1) // PAGE) * PAGE + 100 - Tn      # above the longest, inside the table's last entry
    dl0 = torch.tensor(l0, dtype=torch.int32, device=DEV)
    whole, gots = [], {}
    for program, tile in G.extend_programs(*case):
        pb = extend_problem(dt, Dh, H, Hkv, Tn, len0, program, tile)
        q, kp, vp = pb.q.to(DEV), pb.kp.to(DEV), pb.vp.to(DEV)
        dd = [(k[None, :, :e].contiguous().to(DEV), v[None, :, :e].contiguous().to(DEV)) for (k, v), e in zip(pb.dense, pb.ends)]

        def paged(table, fill):
            ws = None if fill is None else torch.full((ops.attention_extend_paged_workspace(len(l0), Tn, H, Dh, max_len0, Hkv, dt),), fill, device=DEV)
            return ops.attention_extend_paged(q, kp, vp, table, dl0, H, Tn, max_len0, scale, ws=ws)

        def dense(b, m):
            return ops.attention_extend(q[b * Tn:(b + 1) * Tn], dd[b][0], dd[b][1], m[None, :pb.ends[b]].contiguous(), H, Tn, l0[b], scale)

        def ref64(b, m):
            k, v = pb.dense[b]
            return _extend_ref(pb.q[b * Tn:(b + 1) * Tn], k[None], v[None], m[None], H, Hkv, Dh, l0[b], Tn)

        def ref32(b, m):
            k, v = pb.dense[b]
            return G._extend_ref32(pb.q[b * Tn:(b + 1) * Tn], k[None], v[None], m[None], H, Hkv, Dh, l0[b], Tn)

        for case_t in table_cases(pb.P, pb.new0):
            name = f"paged extend {NAME[dt]} Dh={Dh} H={H} Hkv={Hkv} len0={len0} Tn={Tn} {G._label(program, tile)} table={case_t}"
            got = _check_launch(cases, name, dt, Dh, pb, case_t, paged, dense, ref64, ref32)
            (whole if case_t == "whole" else gots.setdefault(case_t, [])).append(got)
    _tables_mattered(cases, f"paged extend {G._case_id(case)}", whole, gots)
    cases.done()
