"""Seeded inputs of the MXFP4 KV cache tests (include/setok_hip.h, "MXFP4 KV cache"), on the CPU: caches quantised by the oracle of the storage
contract (tests/mxfp4_cases.py), their exact fp64 meaning, and the small head-dim-32 model case.  Never the code under test."""
import functools
import os
import re

import torch

import mxfp4_cases as M
import setok_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def define(name):
    """An integer #define of include/setok_hip.h."""
    text = open(os.path.join(ROOT, "include", "setok_hip.h")).read()
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", text).group(1))


def quantize_cache(x):
    """(q (..., Dh/2) uint8, s (..., Dh/32) uint8) of rows x (..., Dh) by the oracle."""
    Dh = x.shape[-1]
    q, s = M.quantize_rows(x.reshape(-1, Dh))
    return q.reshape(x.shape[:-1] + (Dh // 2,)), s.reshape(x.shape[:-1] + (Dh // M.BLOCK,))


def dequant(q, s):
    """K' (fp64, (..., Dh)) of a nibble tensor (..., Dh/2) and its scale bytes (..., Dh/32); NaN where a scale byte is 0xFF."""
    q, s = q.cpu(), s.cpu()
    return M.dequantize_rows(q.reshape(-1, q.shape[-1]), s.reshape(-1, s.shape[-1])).reshape(q.shape[:-1] + (2 * q.shape[-1],))


@functools.lru_cache(maxsize=None)
def cache_rows(B, Hkv, cap, Dh, seed):
    """(k_q, k_s, v_q, v_s) of a seeded cache: Gaussian rows whose blocks have scales over five octaves (the scale bytes differ between the blocks of
    a row and between rows), quantised by the oracle.  Shared between the element types and head counts of a test, never modified (callers clone)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        x = torch.randn(B, Hkv, cap, Dh // M.BLOCK, M.BLOCK, generator=g) * 2.0 ** torch.randint(-2, 3, (B, Hkv, cap, Dh // M.BLOCK, 1), generator=g).float()
        out += list(quantize_cache(x.reshape(B, Hkv, cap, Dh)))
    return tuple(out)


def decode_problem(dt, H, Hkv, Dh, n, cap, seed):
    """The decode problem of the fp8 cache's test over an MXFP4 cache: (qkv, k_q, k_s, v_q, v_s, mask).  Four sequences: all keys, left-padded,
    right-padded, fully masked.  Dead slots (masked, or at / past n) hold nibble bytes 0xFF and scale bytes 0xFF and 0x00 alternately; mask
    bytes past n are 1."""
    B = 4
    qkv = torch.randn(B, (H + 2 * Hkv) * Dh, generator=torch.Generator().manual_seed(seed)).to(dt)
    k_q, k_s, v_q, v_s = [t.clone() for t in cache_rows(B, Hkv, cap, Dh, seed + 1)]
    mask = torch.zeros(B, cap, dtype=torch.uint8)
    mask[0, :n] = 1
    mask[1, n // 3:n] = 1
    mask[2, :n - n // 4] = 1
    mask[:, n:] = 1
    dead = (mask == 0)[:, None, :].expand(B, Hkv, cap).clone()
    dead[:, :, n:] = True
    bad_s = torch.where(torch.arange(cap) % 2 == 0, 0xFF, 0x00).to(torch.uint8)[None, None, :, None].expand(B, Hkv, cap, Dh // M.BLOCK)
    for q, s in ((k_q, k_s), (v_q, v_s)):
        q[dead] = 0xFF
        s[dead] = bad_s[dead]
    return qkv, k_q, k_s, v_q, v_s, mask


# ---- the model case at head dim 32 --------------------------------------------------------------------------------------------------------------
DH32 = dict(hidden_size=128, intermediate_size=160, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=100)
DH32_SEED, DH32_B, DH32_T = 41, 3, 13


def dh32_case():
    """(kwargs, state dict, x, am, pos) of a left-padded fp32 Llama with head dim 32 (one MX block per row, two lanes per row in the decode kernel)."""
    lc = O.LlamaConfigLite(**DH32)
    x, am, pos = O.llama_inputs(lc, DH32_SEED, DH32_B, DH32_T, "left")
    return DH32, O.init_llama_weights(lc, seed=DH32_SEED), x, am, pos


def round_trip(x):
    """x (..., Dh) on any device -> K' of its rows in x's dtype and on x's device (exact): what an MXFP4 cache holds after appending x."""
    q, s = quantize_cache(x.detach().cpu())
    return dequant(q, s).to(device=x.device, dtype=x.dtype)
