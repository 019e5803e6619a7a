"""LoRA adapters on the decoder stack of llama.LlamaModel: the reference's fine-tuning stage (scripts/finetune.sh: --lora_enable True --lora_r 128
--lora_alpha 256; src/train/train_setokim.py:272-288 wraps every nn.Linear of the decoder — q, k, v, o, gate, up, down; lm_head excluded — with
peft's LoraConfig and casts the adapters to the 16-bit type).

An adapted projection computes  y = x W^T + s * (drop(x) A^T) B^T  with s = lora_alpha / r, A (r, in) Kaiming-uniform (a = sqrt(5)) and
B (out, r) zero (peft's defaults), W frozen.  This module holds the parameters (`LoraAdapters`, which LlamaModel keeps as `self.lora`, outside
`self.layers`), the adapter-file key format and the merge; the forward / backward arithmetic is llama_train.llama_lora_forward_train /
llama_lora_backward, whose (rows x r) GEMMs are `ops.linear_skinny` (csrc/gemm_skinny.hip)."""
from __future__ import annotations

import math
from typing import Dict, Iterable, Iterator, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import ops

ALL_SEVEN = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
_ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")
_PEFT_PREFIX = "base_model.model.model.layers."                # PeftModel.base_model (LoraModel) .model (the CausalLM) .model (LlamaModel) .layers


def _block(name: str) -> str:
    return "self_attn" if name in _ATTN else "mlp"


class LoraPair(nn.Module):
    """lora_A (r, in) and lora_B (out, r) of one projection."""

    def __init__(self, r: int, fan_in: int, fan_out: int, dtype, device):
        super().__init__()
        a = torch.empty((r, fan_in), dtype=torch.float32)
        nn.init.kaiming_uniform_(a, a=math.sqrt(5))                         # peft's reset_lora_parameters: U(-1 / sqrt(in), 1 / sqrt(in))
        self.lora_A = nn.Parameter(a.to(device=device, dtype=dtype))
        self.lora_B = nn.Parameter(torch.zeros((fan_out, r), dtype=dtype, device=device))


class LoraAdapters(nn.Module):
    """The adapters of a LlamaModel: `layers[i][target]` is a LoraPair.  `seed` is the dropout seed of the latest training-mode forward
    (None when no mask was drawn); projection (layer, target) draws its mask from counters starting at `dropout_offset(layer, target)`."""

    def __init__(self, model, r: int, lora_alpha: float, targets: Sequence[str], lora_dropout: float):
        super().__init__()
        self.r, self.lora_alpha, self.scaling, self.lora_dropout = int(r), float(lora_alpha), float(lora_alpha) / int(r), float(lora_dropout)
        self.targets = tuple(t for t in ALL_SEVEN if t in targets)
        w0 = model.norm.weight
        self.layers = nn.ModuleList()
        for l in model.layers:
            pairs = nn.ModuleDict()
            for t in self.targets:
                lin = getattr(getattr(l, _block(t)), t)
                pairs[t] = LoraPair(self.r, lin.in_features, lin.out_features, w0.dtype, w0.device)
            self.layers.append(pairs)
        self.seed: Optional[int] = None

    @staticmethod
    def dropout_offset(layer: int, target: str) -> int:
        """First counter of the dropout mask of projection (layer, target): 2^40 counters apart, more than any activation has elements."""
        return (layer * len(ALL_SEVEN) + ALL_SEVEN.index(target)) << 40

    def named_pairs(self) -> Iterator[Tuple[int, str, LoraPair]]:
        for i, pairs in enumerate(self.layers):
            for t in self.targets:
                yield i, t, pairs[t]

    def flat(self):
        """(names, tensors): every lora_A / lora_B in a fixed order, named "{layer}.{target}.lora_A"."""
        names, tensors = [], []
        for i, t, p in self.named_pairs():
            names += [f"{i}.{t}.lora_A", f"{i}.{t}.lora_B"]
            tensors += [p.lora_A, p.lora_B]
        return names, tensors


def check_request(model, r, lora_alpha, target_modules: Iterable[str], lora_dropout) -> Tuple[str, ...]:
    """add_lora_'s refusals, each by name.  Returns the targets in canonical order."""
    if getattr(model, "lora", None) is not None:
        raise NotImplementedError("LlamaModel.add_lora_: adapters are already attached (a second set is not implemented; merge_lora_() first)")
    if model.weight_format != "native":
        tag = model.weight_format.split("_")[0]                                     # "fp8_e4m3" -> "fp8", "mxfp4_e2m1" -> "mxfp4"
        raise NotImplementedError(f"LlamaModel.add_lora_: the stack is in {tag} storage (quantize_{tag}_), which is inference-only; attach "
                                  "adapters to the native weights")
    targets = tuple(target_modules)
    unknown = [t for t in targets if t not in ALL_SEVEN]
    if unknown or not targets:
        raise ValueError(f"LlamaModel.add_lora_: unknown target_modules {unknown or list(targets)}; the adaptable projections are {list(ALL_SEVEN)}")
    gran = ops.k_align(model.norm.weight.dtype)
    if isinstance(r, bool) or not isinstance(r, int) or r < gran or r % gran != 0 or r > ops.SKINNY_MAX_N // 2:
        raise ValueError(f"LlamaModel.add_lora_: r={r!r} must be a positive multiple of {gran}, the GEMM's K granule in {model.norm.weight.dtype}, "
                         f"and at most {ops.SKINNY_MAX_N // 2}")
    if not 0.0 <= float(lora_dropout) < 1.0:
        raise ValueError(f"LlamaModel.add_lora_: lora_dropout={lora_dropout!r} must be in [0, 1)")
    if not float(lora_alpha) > 0.0:
        raise ValueError(f"LlamaModel.add_lora_: lora_alpha={lora_alpha!r} must be positive")
    return tuple(t for t in ALL_SEVEN if t in targets)


def state_dict_of(adapters: LoraAdapters) -> Dict[str, torch.Tensor]:
    """peft's adapter-file keys: base_model.model.model.layers.{i}.{self_attn|mlp}.{target}.lora_{A|B}.weight (the adapter name is cut out of the
    saved keys).  peft is not installed where this was written: the format is taken from the reference's save and load code
    (train_setokim.py:430-440 saves the parameters whose name holds "lora_" through save_pretrained, builder.py:76-83 loads them with
    PeftModel.from_pretrained) and has NOT been checked against a peft-written file."""
    out = {}
    for i, t, p in adapters.named_pairs():
        base = f"{_PEFT_PREFIX}{i}.{_block(t)}.{t}."
        out[base + "lora_A.weight"] = p.lora_A.detach()
        out[base + "lora_B.weight"] = p.lora_B.detach()
    return out


@torch.no_grad()
def load_state_dict_into(adapters: LoraAdapters, sd: Dict[str, torch.Tensor]) -> None:
    """The keys of state_dict_of, or the in-memory spelling with the adapter name (`...lora_A.default.weight`).  Every adapter tensor must be
    present with its shape and no other key may be: KeyError / ValueError naming the key."""
    want = {}
    for i, t, p in adapters.named_pairs():
        base = f"{_PEFT_PREFIX}{i}.{_block(t)}.{t}."
        want[base + "lora_A.weight"] = p.lora_A
        want[base + "lora_B.weight"] = p.lora_B
    seen = set()
    for k, v in sd.items():
        key = k.replace(".lora_A.default.", ".lora_A.").replace(".lora_B.default.", ".lora_B.")
        if key not in want:
            raise KeyError(f"load_lora_state_dict: unexpected key {k!r} (the adapters cover {adapters.targets} of {len(adapters.layers)} layers)")
        if tuple(v.shape) != tuple(want[key].shape):
            raise ValueError(f"load_lora_state_dict: {k!r} has shape {tuple(v.shape)}, the adapter {tuple(want[key].shape)}")
        want[key].copy_(v.to(device=want[key].device, dtype=want[key].dtype))
        seen.add(key)
    missing = sorted(set(want) - seen)
    if missing:
        raise KeyError(f"load_lora_state_dict: missing keys {missing[:4]}{' ...' if len(missing) > 4 else ''}")


@torch.no_grad()
def merge_into(model) -> None:
    """W <- W + s * B A for every adapted projection: the product in fp32 (one GEMM over K = r, fp32 out), the sum in fp32, one rounding."""
    ad = model.lora
    for i, t, p in ad.named_pairs():
        lin = getattr(getattr(model.layers[i], _block(t)), t)
        delta = ops.linear(p.lora_B.detach().contiguous(), ops.transpose(p.lora_A.detach().contiguous()), out_dtype=torch.float32)     # (out, in)
        lin.weight.copy_((lin.weight.float() + ad.scaling * delta).to(lin.weight.dtype))
