"""What tests/test_rowwise_gpu.py asserts can be met and cannot be slipped past — checked on the CPU with the verdicts of tests/rowwise_cases.py:
for every case of the GPU module (a) an fp32 emulation of the kernel's formula, with its roundings, comes out clean: the bars are attainable by the
arithmetic; (b) every slip of the op's family — the same emulation wrong in one way — is caught by at least one case.  A slip no case catches is a
missing case."""
import pytest
import torch

import rowwise_cases as RC

IDS = [RC.NAME[d] for d in RC.DTS]


class _Slips:
    """Runs a family's slips over its cases until each is caught once."""

    def __init__(self, slips):
        self.open = list(slips)

    def try_each(self, verdict_of):
        """verdict_of(slip) -> a Findings filled by the case's verdict on the slipped result (None: the slip does not apply to this case)."""
        for slip in list(self.open):
            f = verdict_of(slip)
            if f is not None and f.bad:
                self.open.remove(slip)

    def done(self):
        assert not self.open, f"no case catches: {self.open}"


@pytest.mark.parametrize("dt", RC.DTS, ids=IDS)
def test_rmsnorm_forward_bars_attainable_and_slips_caught(dt):
    clean, slips = RC.Findings(), _Slips(RC.RMS_SLIPS if dt != RC.F32 else [s for s in RC.RMS_SLIPS if s != "no_rnd_w"])
    for rows, C in RC.RMS_GENERIC + RC.RMS_ROWS:
        x, w32 = RC.rms_inputs(rows, C, dt)
        x = x[RC.rms_checked_rows(rows)]
        label = f"emulated rmsnorm {RC.NAME[dt]} {rows}x{C}"
        RC.rms_verdict(clean, label, RC.rms_emulate(x, w32, dt), x, w32, dt)

        def slipped(slip):
            f = RC.Findings()
            RC.rms_verdict(f, f"{label} {slip}", RC.rms_emulate(x, w32, dt, slip=slip), x, w32, dt)
            return f
        slips.try_each(slipped)
    print(f"worst per-row error of the emulation, {RC.NAME[dt]}: {clean.worst:.3e}")
    clean.done()
    slips.done()


@pytest.mark.parametrize("dt", RC.DTS, ids=IDS)
def test_rmsnorm_backward_bars_attainable_and_slips_caught(dt):
    clean, slips = RC.Findings(), _Slips(RC.RMS_BWD_SLIPS)
    for rows, C in RC.RMS_BWD:
        x, w32, dy, dres = RC.rms_bwd_inputs(rows, C, dt)
        for r in (None, dres):
            label = f"emulated rmsnorm_bwd {RC.NAME[dt]} {rows}x{C}" + (" +dres" if r is not None else "")
            RC.rms_bwd_verdict(clean, label, RC.rms_bwd_emulate(x, w32, dy, r, dt), x, w32, dy, r, dt)

        def slipped(slip):
            f = RC.Findings()
            RC.rms_bwd_verdict(f, f"{label} {slip}", RC.rms_bwd_emulate(x, w32, dy, dres, dt, slip=slip), x, w32, dy, dres, dt)
            return f
        slips.try_each(slipped)
    print(f"worst per-row error of the emulation, {RC.NAME[dt]}: {clean.worst:.3e}")
    clean.done()
    slips.done()


@pytest.mark.parametrize("dt", RC.DTS, ids=IDS)
def test_rope_bars_attainable_and_slips_caught(dt):
    clean, fwd, bwd = RC.Findings(), _Slips(RC.ROPE_SLIPS), _Slips(RC.ROPE_SLIPS)
    for H, Hkv, Dh in RC.ROPE_HEADS:
        for rows in RC.ROPE_ROWS:
            qkv, pos = RC.rope_inputs(rows, H, Hkv, Dh, dt)
            label = f"emulated rope {RC.NAME[dt]} H{H} Hkv{Hkv} Dh{Dh} rows{rows}"
            y = RC.rope_emulate(qkv, pos, H, Hkv, Dh, dt)
            RC.rope_verdict(clean, label, y, qkv, pos, H, Hkv, Dh, dt)
            RC.rope_verdict(clean, label + " bwd", RC.rope_emulate(qkv, pos, H, Hkv, Dh, dt, backward=True), qkv, pos, H, Hkv, Dh, dt, backward=True)
            clean.rows(label + " there and back", RC.rope_emulate(y, pos, H, Hkv, Dh, dt, backward=True), qkv.double(), 2 * RC.ROPE_TOL[dt])
            for slips, back in ((fwd, False), (bwd, True)):
                def slipped(slip):
                    f = RC.Findings()
                    RC.rope_verdict(f, f"{label} {slip}", RC.rope_emulate(qkv, pos, H, Hkv, Dh, dt, backward=back, slip=slip), qkv, pos, H, Hkv, Dh, dt,
                                    backward=back)
                    return f
                slips.try_each(slipped)
    print(f"worst per-row error of the emulation, {RC.NAME[dt]}: {clean.worst:.3e}")
    clean.done()
    fwd.done()
    bwd.done()


@pytest.mark.parametrize("dt", RC.DTS, ids=IDS)
def test_lm_loss_bars_attainable_and_slips_caught(dt):
    clean, slips = RC.Findings(), _Slips(RC.LM_SLIPS)
    for B, T, V in RC.LM_CASES:
        for padding in ("right", "left"):
            for hot in (False, True):
                logits, labels, am = RC.lm_inputs(B, T, V, padding, hot, dt)
                label = f"emulated lm_loss {RC.NAME[dt]} B{B} T{T} V{V} {padding} {'hot' if hot else 'unit'}"
                out, d = RC.lm_emulate(logits, labels, am, dt)
                RC.lm_verdict(clean, label, out, d, logits, labels, am, dt, hot)

                def slipped(slip):
                    f = RC.Findings()
                    o2, d2 = RC.lm_emulate(logits, labels, am, dt, slip=slip)
                    RC.lm_verdict(f, f"{label} {slip}", o2, d2, logits, labels, am, dt, hot)
                    return f
                slips.try_each(slipped)
    clean.done()
    slips.done()


@pytest.mark.parametrize("dt", RC.DTS, ids=IDS)
def test_layernorm_backward_bars_attainable_and_slips_caught(dt):
    clean, slips = RC.Findings(), _Slips(RC.LN_SLIPS)
    for rows, C, dts in RC.LN_CASES:
        if dt not in dts:
            continue
        assert C <= RC.ln_limit(dt)
        x, dy, res, gamma = RC.ln_inputs(rows, C, dt)
        label = f"emulated layernorm_bwd {RC.NAME[dt]} {rows}x{C}"
        RC.ln_verdict(clean, label, *RC.ln_emulate(x, dy, res, gamma, dt), x, dy, res, gamma, dt)

        def slipped(slip):
            f = RC.Findings()
            RC.ln_verdict(f, f"{label} {slip}", *RC.ln_emulate(x, dy, res, gamma, dt, slip=slip), x, dy, res, gamma, dt)
            return f
        slips.try_each(slipped)
    assert any(C == RC.ln_limit(dt) for _, C, dts in RC.LN_CASES if dt in dts)           # the limit itself is a case
    print(f"worst per-row error of the emulation, {RC.NAME[dt]}: {clean.worst:.3e}")
    clean.done()
    slips.done()


@pytest.mark.parametrize("dt", RC.DTS, ids=IDS)
def test_colsum_bar_attainable_and_slip_caught(dt):
    clean, caught = RC.Findings(), 0
    seen = set()
    for rows in RC.COLSUM_ROWS:
        seen.add(RC.colsum_plan(rows)[0])
        for cols in RC.COLSUM_COLS:
            x = RC.colsum_inputs(rows, cols, dt)
            label = f"emulated colsum {RC.NAME[dt]} {rows}x{cols}"
            RC.colsum_verdict(clean, label, RC.colsum_emulate(x), x)
            f = RC.Findings()
            RC.colsum_verdict(f, label + " last_chunk", RC.colsum_emulate(x, slip="last_chunk"), x)
            caught += bool(f.bad)
    clean.done()
    assert caught == len(RC.COLSUM_ROWS) * len(RC.COLSUM_COLS)                             # a dropped chunk shows in EVERY case
    # what the final kernel's loops see: one chunk, an even and an odd count per quarter, the 128-chunk cap from both sides, the 512-row branch
    assert seen == {1, 2, 4, 5, 9, 128, 125, 33, 40}, seen
    assert RC.colsum_plan(16384) == (128, 128) and RC.colsum_plan(16385) == (33, 497) and RC.colsum_plan(4097) == (125, 33)


def _elementwise(op, dt, lo, hi, seed):
    """(result in `dt`, float64 reference) of one window of items [lo, hi) of a capped-grid op, from its own seeded inputs."""
    n = hi - lo
    if op == "gelu_bwd":
        pre, dy = (RC.randn(n, seed=seed) * 2).to(dt), RC.randn(n, seed=seed + 1).to(dt)
        x = pre.float()
        got = dy.float() * (0.5 * (1 + torch.erf(x * 0.7071067811865476)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x))
        return got.to(dt), RC.gelu_bwd_ref(pre, dy), 1
    if op == "activation":
        x = (RC.randn(n, seed=seed) * 2).to(dt)
        return torch.nn.functional.gelu(x.float()).to(dt), RC.gelu_ref(x), 1
    if op == "swiglu_pairs_bwd":                                                          # an item: VEC outputs' worth of pairs
        v = RC.vec(dt)
        pairs, dout = (RC.randn(n, 2 * v, seed=seed) * 2).to(dt), RC.randn(n, v, seed=seed + 1).to(dt)
        gate, up, go = pairs.float()[:, 0::2], pairs.float()[:, 1::2], dout.float()
        s = 1.0 / (1.0 + torch.exp(-gate))
        got = torch.stack([go * up * s * (1 + gate * (1 - s)), go * gate * s], -1).reshape(n, 2 * v)
        return got.to(dt), RC.swiglu_pairs_bwd_ref(pairs, dout), 2 * v
    assert op == "adamw"
    h = RC.ADAMW
    p, g, m, v = RC.randn(n, seed=seed), RC.randn(n, seed=seed + 1), 0.1 * RC.randn(n, seed=seed + 2), 0.01 * RC.randn(n, seed=seed + 3).abs()
    gi = g * h["grad_scale"]
    mi = h["beta1"] * m + (1 - h["beta1"]) * gi
    vi = h["beta2"] * v + (1 - h["beta2"]) * gi * gi
    w = p * (1 - h["lr"] * h["weight_decay"]) - h["lr"] * (mi / (1 - h["beta1"] ** h["step"])) / (torch.sqrt(vi / (1 - h["beta2"] ** h["step"])) + h["eps"])
    return w, RC.adamw_ref(p, g, m, v)[0], 1


@pytest.mark.parametrize("op", list(RC.CAP_TOL))
def test_capped_grid_windows_attainable_and_slip_caught(op):
    for dt, tol in RC.CAP_TOL[op].items():
        n_items = RC.CAP + 1000
        clean, caught = RC.Findings(), []
        for i, (lo, hi) in enumerate(RC.windows(n_items)):
            got, ref, per_item = _elementwise(op, dt, lo, hi, seed=31 * i)
            label = f"emulated {op} {RC.NAME[dt]} items {lo}..{hi}"
            RC.window_verdict(clean, label, got, ref, tol)
            f = RC.Findings()
            RC.window_verdict(f, label + " first_cap", RC.cap_slip(got, lo, per_item).reshape(got.shape), ref, tol)
            caught.append(bool(f.bad))
        clean.done()
        assert caught == [False, True, True], caught                                       # the window across item 2^24 and the last one see it
