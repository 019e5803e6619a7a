"""CPU oracle of the MXFP4 weight-only storage contract (include/setok_hip.h, "MXFP4 weight-only decode") and the seeded inputs of its tests.
Pure torch on the CPU, in float64; never the code under test.

A matrix W (N, K), K % 32 == 0, is stored as q (N, K/2) bytes of two e2m1 nibbles (element 2j low, 2j+1 high) + s (N, K/32) e8m0 scale bytes and
means exactly W'[n, k] = value(nibble[n, k]) * 2^(s[n, k/32] - 127); a block whose scale byte is 0xFF is 32 NaNs."""
import torch

import llama_bwd_cases as C
import setok_oracle as O

BLOCK, E_MIN, E_MAX, BIAS, NAN_SCALE = 32, -13, 13, 127, 0xFF
VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)                # magnitude codes 0..7; bit 3 of a nibble is the sign
# the rounding, as an explicit table: (midpoint between code i and code i + 1, does a value exactly there go UP?) — up where code i + 1 is even
MIDPOINTS = ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False))


def quantize_rows(W):
    """(q uint8 (N, K/2), s uint8 (N, K/32)) of a CPU matrix in fp32 / bf16 / fp16, by the rule of the header, per block of 32 elements of a row:
    a non-finite entry -> scale byte 0xFF, nibbles 0;  amax == 0 -> scale byte 127;  else e = floor(log2(amax)) - 2 by frexp (amax = m * 2^x,
    m in [0.5, 1): floor(log2) = x - 1), clamped to [-13, 13];  nibble = sign bit of W | code of min(|W| * 2^-e, 6) by MIDPOINTS."""
    w = W.detach().cpu().double()                                  # exact for all three types, and so is every power-of-two scaling below
    N, K = w.shape
    assert K % BLOCK == 0
    b = w.view(N, K // BLOCK, BLOCK)
    finite = torch.isfinite(b).all(dim=-1)
    b0 = torch.where(finite[..., None], b, torch.zeros_like(b))
    amax = b0.abs().amax(dim=-1)
    _, x = torch.frexp(amax)
    e = (x - 3).clamp(E_MIN, E_MAX)
    e = torch.where(amax > 0, e, torch.zeros_like(e)).to(torch.int32)
    a = torch.ldexp(b0.abs(), -e[..., None]).clamp(max=6.0)
    code = torch.zeros_like(a, dtype=torch.int32)
    for mid, up in MIDPOINTS:
        code += ((a >= mid) if up else (a > mid)).to(torch.int32)
    nib = code | (torch.signbit(b0).to(torch.int32) << 3)
    nib = torch.where(finite[..., None], nib, torch.zeros_like(nib)).view(N, K)
    q = (nib[:, 0::2] | (nib[:, 1::2] << 4)).to(torch.uint8)
    s = torch.where(finite, e + BIAS, torch.full_like(e, NAN_SCALE)).to(torch.uint8)
    return q, s


def nibbles(q):
    """(N, K) int32 nibbles of q (N, K/2)."""
    q = q.cpu().to(torch.int32)
    return torch.stack([q & 15, q >> 4], dim=-1).view(q.shape[0], -1)


def dequantize_rows(q, s):
    """W' in fp64: value(nibble) * 2^(s - 127); NaN where the scale byte is 0xFF."""
    nib = nibbles(q)
    mag = torch.tensor(VALUES, dtype=torch.float64)[nib & 7]
    val = torch.where((nib & 8) != 0, -mag, mag)
    sc = s.cpu().to(torch.int32)
    w = torch.ldexp(val.view(q.shape[0], -1, BLOCK), (sc - BIAS)[..., None])
    w = torch.where((sc == NAN_SCALE)[..., None], torch.full_like(w, float("nan")), w)
    return w.view(q.shape[0], -1)


TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


def special_blocks(dtype, seed):
    """(10, 32) in `dtype`: the blocks the quantiser can get wrong.  0 all zeros; 1 amax 0.8 * 2^-13 (e = -16 clamps at -13: results 0, 0.5, 1);
    2 amax 1e5 (e = 14 clamps at 13, saturating; fp16 holds 6e4 at most, so there the block peaks at 60000: e = 13, still saturating); 3 amax exactly
    6 * 2^-3 (e = -3, the code of 6, nothing saturates); 4 amax one ulp of the type below 8 * 2^-3 = 1 (e = -3, 7.99.. saturates to 6); 5 every tie of
    the e2m1 grid at e = 0 in both signs under an amax of 6; 6 negative zero and negatives that round to zero under an amax of 4; 7 and 8 neighbours
    whose scales are 20 octaves apart (amax in [2^10, 2^11) next to amax in [2^-10, 2^-9)); 9 a Llama-like Gaussian block."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda: torch.randn(BLOCK, generator=g).double()
    unit = lambda: (lambda r: r / r.abs().max())(rnd())
    blocks = [torch.zeros(BLOCK).double(), unit() * 0.8 * 2.0 ** -13, unit() * (6e4 if dtype == torch.float16 else 1e5), unit() * 0.7, unit() * 0.7,
              unit() * 0.2, unit() * 3.9, unit() * 1500.0, unit() * 1500.0 * 2.0 ** -20, rnd() * 0.02]
    blocks[3][7] = 0.75
    blocks[4][7] = float(torch.nextafter(torch.tensor(1.0, dtype=dtype), torch.tensor(0.0, dtype=dtype)))
    blocks[5][:15] = torch.tensor(list(TIES) + [-t for t in TIES] + [6.0]).double()
    blocks[6][:5] = torch.tensor([-0.0, -0.1, -0.25, 4.0, -0.2501]).double()
    return torch.stack(blocks).to(dtype)


def special_rows(K, dtype, seed, rows=None):
    """(rows, K) in `dtype`: the special blocks laid along the rows, block b of row r being special block (r * K/32 + b) % 10 — so at five or
    more blocks per row the 20-octave neighbours share a row.  Default: as many rows as show every block once."""
    nb = K // BLOCK
    sp = special_blocks(dtype, seed)
    rows = -(-sp.shape[0] // nb) if rows is None else rows
    idx = (torch.arange(rows * nb) % sp.shape[0]).view(rows, nb)
    return sp[idx].reshape(rows, K)


def quantizer_matrix(N, K, dtype, seed=0):
    """(N, K) in `dtype`: rows of special blocks (the even rows) with seeded Gaussian rows between them whose blocks have scales 1e-4 .. 1e2."""
    g = torch.Generator().manual_seed(1000 + seed)
    sp = special_rows(K, dtype, seed, rows=(N + 1) // 2)
    rows = []
    for n in range(N):
        if n % 2 == 0:
            rows.append(sp[n // 2])
        else:
            scale = 10.0 ** torch.randint(-4, 3, (K // BLOCK, 1), generator=g).double()
            rows.append((torch.randn(K // BLOCK, BLOCK, generator=g).double() * scale).reshape(K).to(dtype))
    return torch.stack(rows)


def gemm_problem(M, N, K, dtype, seed):
    """(a (M, K) in `dtype`, q, s, W' in fp64, residual (M, N) in `dtype`): seeded Llama-like weights (std 0.02 with per-block scales over four
    octaves, so the scale bytes differ between the blocks of a row and between rows) quantised by the oracle, unit-scale activations."""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(N, K // BLOCK, BLOCK, generator=g) * 0.02 * (2.0 ** torch.randint(-2, 3, (N, K // BLOCK, 1), generator=g).float())
    q, s = quantize_rows(W.view(N, K))
    a = torch.randn(M, K, generator=g).to(dtype)
    r = torch.randn(M, N, generator=g).to(dtype)
    return a, q, s, dequantize_rows(q, s), r


def quantized_state_dict(sd, dtype=torch.float32):
    """The state dict (fp32) of the Llama whose stack projections lie on the MXFP4 grid: every `model.layers.*_proj.weight` replaced by the oracle's
    W' of that weight AS A MODEL IN `dtype` HOLDS IT.  W' is exact in fp32 and in `dtype`.  Blocks lie along K inside a row, so quantising the
    parts equals quantising the fused matrices the model packs."""
    out = {}
    for k, v in sd.items():
        if k.startswith("model.layers.") and k.endswith("_proj.weight"):
            out[k] = dequantize_rows(*quantize_rows(v.float().to(dtype))).float()
        else:
            out[k] = v.clone()
    return out


# ---- the model cases ---------------------------------------------------------------------------------------------------------------------------
# The tiny cases of llama_bwd_cases.py have intermediate 176, which holds no whole number of blocks: one small fp32 case of this file's own.
MX_CASES = {
    # name: (LlamaConfigLite kwargs, seed, B, T, padding)
    "mx_tiny_left": (dict(hidden_size=64, intermediate_size=160, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=100), 31, 3, 13, "left"),
}


def case_inputs(name):
    """llama_bwd_cases.case_inputs, extended by MX_CASES: (kw, lc, seed, x, am, pos)."""
    if name not in MX_CASES:
        return C.case_inputs(name)[:6]
    kw, seed, B, T, padding = MX_CASES[name]
    lc = O.LlamaConfigLite(**kw)
    x, am, pos = O.llama_inputs(lc, seed, B, T, padding)
    return kw, lc, seed, x, am, pos
