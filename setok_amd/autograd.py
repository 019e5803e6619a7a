"""Autograd through the drop-in boundary.

The reference's main caller of `encode_images` is a TRAINING forward: stage 2 trains `mm_in_projector` through the LLM loss with the
tokenizer frozen (scripts/pretrain_mm_proj.sh:40, src/train/train_setokim.py:336-339), the projected tokens travel through
`prepare_inputs_labels_for_multimodal` into `inputs_embeds` (src/model/setokim_arch.py:206-211,290-293) and torch autograd carries
dL/dinputs_embeds back.  Stage 1 trains the tokenizer's head itself.  The reference gets all of that for free from torch ops; the modules
here run on the HIP library, so the three places where a gradient has to cross the library are `torch.autograd.Function`s whose backward
is made of the same entry points the hand-written training step uses (setok_linear for dX, the split-K `linear_tn` for dW, setok_colsum
inside the transposes for db, setok_gelu_bwd, setok_layernorm_bwd, setok_splice_rows_bwd, training.head_backward):

    ProjectorFn   VisionProjector / LinearProjector              d loss / d projector parameters, d loss / d tokens
    SpliceRowsFn  splice_multimodal (the embedding + image rows)    d loss / d projected image tokens (d embed_tokens.weight on request)
    HeadFn        SetokTokenizer.encode_features                    d loss / d head parameters (inner_encoder, inter_encoder, out)
    DetokFn       SetokDeTokenizer.forward / decode_image /         d loss / d decoder parameters, d loss / d tokens (detok_train.py)
                  reconstruction_loss
    LlamaFn       LlamaModel.forward with the decoder stack frozen  d loss / d inputs_embeds across the decoder layers (llama_train.py;
    LlamaLMFn     SetokimLlamaPrefill.forward (logits, LM loss)     the LLM's own weights get no gradient: stage 2 freezes them)
    LlamaLoraFn   the same two with LoRA adapters attached (lora.py)  d loss / d inputs_embeds and every adapter's dA, dB: the reference's
    LlamaLoraLMFn                                                   finetune stage (llama_train.llama_lora_backward)

With them `loss.backward()` on SetokimLlamaPrefill's language-model loss reaches the projector: stage 2 end to end.
Everything else on the path is inference-only and says so (round 4): the forward always runs — reference-style inference callers
do not wrap their calls in no_grad and freshly built modules have trainable parameters — and, when torch would have recorded a graph, the
outputs carry a grad_fn whose backward RAISES (`no_backward`), so nothing trains silently.  The CLIP tower, whose reference forward is itself
`@torch.no_grad()`, warns once and proceeds.  `refuse_grad` (raise at the call) is left for inputs a caller explicitly marked as needing a
gradient that cannot be delivered.  The forward values are the inference
path's, bit for bit, for the projector and the splice; the head's training forward keeps its pre-activation (training.py)."""
from __future__ import annotations

from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from . import ops
from ._packcache import f32_of


def grad_needed(*tensors) -> bool:
    """Would torch autograd record a graph for an op over these tensors?"""
    if not torch.is_grad_enabled():
        return False
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.requires_grad:
            return True
    return False


def refuse_grad(what: str, tensors: Iterable[Any], hint: str = "") -> None:
    """The loud guard for an INPUT a caller explicitly asked a gradient for and cannot get (features handed to the head's training step with
    `requires_grad=True`, ...): raising at the call is the only honest answer there."""
    if not torch.is_grad_enabled():
        return
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise NotImplementedError(
                f"{what} runs on the HIP library without an autograd graph, but gradients are enabled and one of its inputs / parameters "
                f"requires a gradient: the result would silently train nothing.  Freeze it (`requires_grad_(False)`, what the reference's "
                f"stage-2 recipe does for everything but mm_in_projector) or call it under `torch.no_grad()`." + (" " + hint if hint else ""))


class _NoBackwardFn(torch.autograd.Function):
    """Identity whose backward raises: the grad_fn of an inference-only module's output when autograd would have expected a graph."""

    @staticmethod
    def forward(ctx, out, what, msg, *deps):
        ctx.what, ctx.msg = what, msg
        return out.view_as(out)

    @staticmethod
    def backward(ctx, *grads):
        if ctx.msg:
            raise NotImplementedError(ctx.msg)
        raise NotImplementedError(
            f"{ctx.what} ran on the HIP library without an autograd graph (it has no backward pass there): backward() through its output "
            f"would silently train nothing.  Freeze the module (`requires_grad_(False)`), call it under `torch.no_grad()`, or detach its output.")


def no_backward(what: str, value, deps: Iterable[Any], msg: Optional[str] = None):
    """Inference-only modules whose REFERENCE counterpart is differentiable (Block, SetokDeTokenizer, the LLM prefill): the forward runs as
    inference whatever the grad mode — a freshly built nn.Module has `requires_grad=True` parameters and reference-style inference callers do
    not wrap their calls — and, where torch would have recorded a graph (gradients enabled + an input / parameter requiring one),
    every floating-point tensor of the result carries a grad_fn that RAISES in backward.  Nothing trains silently, nothing that only wants the
    values crashes.  `msg`: the backward's error message, when the generic one does not say why."""
    if not torch.is_grad_enabled():
        return value
    live = [t for t in deps if isinstance(t, torch.Tensor) and t.requires_grad]
    if not live:
        return value

    def wrap(v):
        if isinstance(v, torch.Tensor):
            return _NoBackwardFn.apply(v, what, msg, *live) if v.is_floating_point() else v
        if isinstance(v, tuple):
            return tuple(wrap(u) for u in v)
        if isinstance(v, list):
            return [wrap(u) for u in v]
        if isinstance(v, dict):
            return {k: wrap(u) for k, u in v.items()}
        return v
    return wrap(value)


_WARNED: set = set()


def warn_no_grad_once(what: str, tensors: Iterable[Any], why: str, owner: Any = None, inputs: Iterable[Any] = ()) -> None:
    """For a module whose REFERENCE forward is itself `@torch.no_grad()` (the CLIP tower, clip_encoder.py:50): parameters that require a
    gradient get none there either, so the call proceeds exactly like the reference's — with one warning PER MODULE INSTANCE (`owner`; keyed
    by name alone, a second tower with unfrozen parameters went through silently: ADVICE r04) saying so.  `inputs` (e.g. the images) that
    require a gradient get a warning of their own, worded for what it is."""
    if not torch.is_grad_enabled():
        return
    import warnings
    key = (what, id(owner) if owner is not None else None)
    if key + ("params",) not in _WARNED:
        for t in tensors:
            if isinstance(t, torch.Tensor) and t.requires_grad:
                _WARNED.add(key + ("params",))
                warnings.warn(f"{what}: gradients are enabled and a parameter requires one, but {why}; running without a graph.", UserWarning, stacklevel=3)
                break
    if key + ("inputs",) not in _WARNED:
        for t in inputs:
            if isinstance(t, torch.Tensor) and t.requires_grad:
                _WARNED.add(key + ("inputs",))
                warnings.warn(f"{what}: an INPUT requires a gradient, but {why}; no gradient will reach it.", UserWarning, stacklevel=3)
                break


def _grad_as(g: Optional[torch.Tensor], like: torch.Tensor) -> Optional[torch.Tensor]:
    if g is None:
        return None
    return g.to(like.dtype).reshape(like.shape)


# ----------------------------------------------------------------------------------------------------------------------------
# mm_in_projector (src/model/multimodal_projector/builder.py:33-59): Linear [LayerNorm] (GELU Linear)*
# ----------------------------------------------------------------------------------------------------------------------------
class ProjectorFn(torch.autograd.Function):
    """y = projector(x) over rows.  `plan`: tuple of ("linear", fused_gelu, has_bias) | ("ln", eps) | ("gelu",) in module order; `tensors`:
    the parameters in that order (weight, bias per Linear / LayerNorm; a missing bias is simply absent)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, plan: Tuple, owner, *tensors: torch.Tensor):
        h = x.contiguous()
        saved: List[torch.Tensor] = []
        i = 0
        for li, step in enumerate(plan):
            saved.append(h)
            if step[0] == "linear":
                w = tensors[i].detach().contiguous(); i += 1
                b = None
                if step[2]:
                    b = f32_of(owner, f"autograd_bias_{li}", tensors[i]); i += 1
                h = ops.linear(h, w, b, act=ops.ACT_GELU_ERF if step[1] else ops.ACT_NONE)      # the inference path's call: same bits
            elif step[0] == "ln":
                h = ops.layernorm(h, f32_of(owner, f"autograd_lnw_{li}", tensors[i]), f32_of(owner, f"autograd_lnb_{li}", tensors[i + 1]), step[1]); i += 2
            else:
                h = ops.activation(h, ops.ACT_GELU_ERF)
        ctx.plan, ctx.owner, ctx.saved, ctx.tensors = plan, owner, saved, tensors
        return h

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        from .training import linear_bwd
        plan, owner, saved, tensors = ctx.plan, ctx.owner, ctx.saved, ctx.tensors
        need_x = ctx.needs_input_grad[0]
        need_t = ctx.needs_input_grad[3:]
        grads: List[Optional[torch.Tensor]] = [None] * len(tensors)
        # parameter index of every step
        first, i = [], 0
        for step in plan:
            first.append(i)
            i += (1 + (1 if step[2] else 0)) if step[0] == "linear" else (2 if step[0] == "ln" else 0)
        g = dy.to(saved[-1].dtype).contiguous()
        for li in reversed(range(len(plan))):
            step, h, p0 = plan[li], saved[li], first[li]
            need_dx = need_x or any(need_t[:p0])                      # anything upstream still wants a gradient?
            if step[0] == "linear":
                w = tensors[p0].detach().contiguous()
                if step[1]:                                           # fused GELU: the pre-activation is recomputed (one GEMM over sum L_i rows)
                    b = f32_of(owner, f"autograd_bias_{li}", tensors[p0 + 1]) if step[2] else None
                    pre = ops.linear(h, w, b)
                    g = ops.gelu_bwd(pre, g)
                need_dw = need_t[p0] or (step[2] and need_t[p0 + 1])
                gd: Dict[str, torch.Tensor] = {}
                g_in = linear_bwd(h, w, g, gd, "l", need_dx=need_dx, need_dw=need_dw)
                if need_dw:
                    grads[p0] = _grad_as(gd["l.weight"], tensors[p0])
                    if step[2]:
                        grads[p0 + 1] = _grad_as(gd["l.bias"], tensors[p0 + 1])
                g = g_in
            elif step[0] == "ln":
                C = h.shape[1]
                dgam = torch.empty((C,), dtype=torch.float32, device=h.device); dbet = torch.empty_like(dgam)
                g = ops.layernorm_bwd(h, g, f32_of(owner, f"autograd_lnw_{li}", tensors[p0]), step[1], dgam, dbet, accumulate=False, need_dx=need_dx)
                grads[p0], grads[p0 + 1] = _grad_as(dgam, tensors[p0]), _grad_as(dbet, tensors[p0 + 1])
            else:
                g = ops.gelu_bwd(h, g) if need_dx else None
            if g is None:
                break
        return (g if need_x else None, None, None) + tuple(grads)


def projector_plan(mods: Sequence[torch.nn.Module]):
    """(plan, parameter tensors) of an nn.Sequential-style projector for ProjectorFn."""
    import torch.nn as nn
    plan, tensors = [], []
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.Linear):
            fuse = i + 1 < len(mods) and isinstance(mods[i + 1], nn.GELU)
            plan.append(("linear", fuse, m.bias is not None))
            tensors.append(m.weight)
            if m.bias is not None:
                tensors.append(m.bias)
            i += 2 if fuse else 1
        elif isinstance(m, nn.LayerNorm):
            plan.append(("ln", m.eps, True))
            tensors += [m.weight, m.bias]
            i += 1
        elif isinstance(m, nn.GELU):
            plan.append(("gelu", False, False))
            i += 1
        else:
            raise TypeError(f"unsupported projector module {type(m).__name__}")
    return tuple(plan), tensors


# ----------------------------------------------------------------------------------------------------------------------------
# the row copies of prepare_inputs_labels_for_multimodal (setokim_arch.py:266,284,290-303)
# ----------------------------------------------------------------------------------------------------------------------------
class SpliceRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, packed: Optional[torch.Tensor], embed_weight: torch.Tensor, src: torch.Tensor):
        ctx.src = src
        ctx.n_rows = 0 if packed is None else packed.shape[0]
        ctx.vocab = embed_weight.shape[0]
        return ops.splice_rows(src, embed_weight.detach().contiguous(), packed if (packed is not None and packed.shape[0]) else None)

    @staticmethod
    def backward(ctx, d_out: torch.Tensor):
        need_p, need_e = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        d_out = d_out.contiguous()
        dfe, dem = ops.splice_rows_bwd(ctx.src, d_out, ctx.n_rows if need_p else 0, ctx.vocab if need_e else 0)
        if need_p and dfe is None:
            dfe = d_out.new_zeros((0, d_out.shape[-1]))
        return dfe, (dem.to(d_out.dtype) if dem is not None else None), None


# ----------------------------------------------------------------------------------------------------------------------------
# the trainable head of the tokenizer (tokenizer.py:162-180; the tower is frozen and the clustering is no_grad, tokenizer.py:79)
# ----------------------------------------------------------------------------------------------------------------------------
class HeadFn(torch.autograd.Function):
    """tokens = head(hidden_rows) with the activations of training.head_forward_train kept for training.head_backward.  `aux` receives the
    non-differentiable results (counts, idx_cluster, score)."""

    @staticmethod
    def forward(ctx, tok, hidden_rows: torch.Tensor, B: int, k, threshold, noise, token_mask, dropout_seed, aux: dict, names: Tuple[str, ...],
                *params: torch.Tensor):
        from .training import head_forward_train
        tokens, saved = head_forward_train(tok, hidden_rows, B, k, threshold, noise, dropout_seed=dropout_seed, token_mask=token_mask)
        aux.update(counts=list(tokens.counts), idx=saved.pop("idx"), score=saved.pop("score"))
        ctx.tok, ctx.saved, ctx.names, ctx.params = tok, saved, names, params
        return tokens.packed

    @staticmethod
    def backward(ctx, dtokens: torch.Tensor):
        from .training import head_backward
        grads = head_backward(ctx.tok, ctx.saved, dtokens.contiguous())
        out = tuple(_grad_as(grads.get(n), p) for n, p in zip(ctx.names, ctx.params))
        return (None,) * 10 + out


def head_apply(tok, hidden_rows: torch.Tensor, B: int, k=None, threshold=None, noise=None, token_mask=None):
    """(packed tokens with a grad_fn, counts, idx_cluster (B, N), score (B, N)).  Dropout follows the module's mode like the reference's
    nn.Dropout (module.py:36,44,45,59,72): `tok.training` -> the proj_drop masks are active, seeded from torch's default CPU generator
    (`torch.manual_seed` makes a run repeatable); eval mode -> identity."""
    from .training import HEAD_MODULES
    named = [(n, p) for n, p in tok.named_parameters() if n.split(".")[0] in HEAD_MODULES]
    seed = None
    if tok.training and any(getattr(b, "proj_drop_p", 0.0) > 0.0 or getattr(b, "attn_drop_p", 0.0) > 0.0 for b in (tok.inner_encoder, tok.inter_encoder)):
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
    aux: dict = {}
    packed = HeadFn.apply(tok, hidden_rows, B, k, threshold, noise, token_mask, seed, aux, tuple(n for n, _ in named), *[p for _, p in named])
    return packed, aux["counts"], aux["idx"], aux["score"]


# ----------------------------------------------------------------------------------------------------------------------------
# the reconstruction decoder (detokenizer.py; the reference trains it with the tokenizer in one graph, model.py:86-92)
# ----------------------------------------------------------------------------------------------------------------------------
class DetokFn(torch.autograd.Function):
    """SetokDeTokenizer's forward ("feats"), decode_image ("image") or reconstruction_loss ("loss") on packed tokens, keeping what
    detok_train.detok_backward needs.  `names`: the reference names of `params`, in order."""

    @staticmethod
    def forward(ctx, det, mode: str, counts, kind: str, packed: torch.Tensor, gold: Optional[torch.Tensor], names: Tuple[str, ...],
                *params: torch.Tensor):
        saved: Dict[str, Any] = {}
        out = det._compute(packed.detach(), counts, mode, gold, kind, saved=saved)
        ctx.det, ctx.saved, ctx.names, ctx.params = det, saved, names, params
        return out

    @staticmethod
    def backward(ctx, g: torch.Tensor):
        from .detok_train import detok_backward
        need = {n: bool(r) for n, r in zip(ctx.names, ctx.needs_input_grad[7:])}
        dtokens, grads = detok_backward(ctx.det, ctx.saved, g, need_tokens=ctx.needs_input_grad[4], need=need)
        ctx.saved = None
        out = tuple(_grad_as(grads.get(n), p) if need[n] else None for n, p in zip(ctx.names, ctx.params))
        return (None, None, None, None, dtokens, None, None) + out


# ----------------------------------------------------------------------------------------------------------------------------
# the frozen LLM (llama.py): stage 2 trains mm_in_projector THROUGH it (train_setokim.py:335-339), so only d / d inputs_embeds exists
# ----------------------------------------------------------------------------------------------------------------------------
def _spent(what: str):
    return RuntimeError(f"{what}: the saved activations were released by the first backward pass (run the forward again; retain_graph is not supported)")


class LlamaFn(torch.autograd.Function):
    """hidden = LlamaModel(inputs_embeds) with every decoder-stack parameter frozen: the prefill's calls, the prefill's bits, with the
    activations llama_train.llama_backward needs kept."""

    @staticmethod
    def forward(ctx, model, inputs_embeds: torch.Tensor, attention_mask, position_ids):
        from .llama_train import llama_forward_train
        hidden, saved = llama_forward_train(model, inputs_embeds.detach(), attention_mask, position_ids)
        ctx.model, ctx.saved, ctx.like = model, saved, inputs_embeds
        return hidden

    @staticmethod
    def backward(ctx, dhidden: torch.Tensor):
        from .llama_train import llama_backward
        if ctx.saved is None:
            raise _spent("LlamaModel.forward")
        saved, ctx.saved = ctx.saved, None
        dx = llama_backward(ctx.model, saved, dhidden) if ctx.needs_input_grad[1] else None
        like, ctx.like = ctx.like, None
        return None, _grad_as(dx, like), None, None


class LlamaLMFn(torch.autograd.Function):
    """(logits, loss) = SetokimLlamaPrefill's LLM + lm_head (+ the language-model loss when `labels` is given, else a zero) on inputs_embeds,
    with the decoder stack and lm_head frozen.  backward: d loss / d logits (setok_lm_loss_bwd) plus any gradient sent to the logits
    themselves -> lm_head dX -> llama_backward."""

    @staticmethod
    def forward(ctx, prefill, inputs_embeds: torch.Tensor, attention_mask, position_ids, labels):
        from .llama_train import llama_forward_train
        model = prefill.model
        hidden, saved = llama_forward_train(model, inputs_embeds.detach(), attention_mask, position_ids)
        B, T, D = hidden.shape
        w = prefill.lm_head.weight.detach().contiguous()
        logits = ops.linear(hidden.reshape(B * T, D), w).reshape(B, T, -1)
        loss_out = ops.lm_loss(logits, labels, attention_mask) if labels is not None else None
        ctx.prefill, ctx.saved, ctx.like = prefill, saved, inputs_embeds
        ctx.lm = (logits, labels, attention_mask, loss_out)
        ctx.set_materialize_grads(False)
        return logits, (loss_out[0].clone() if loss_out is not None else logits.new_zeros((), dtype=torch.float32))

    @staticmethod
    def backward(ctx, dlogits: Optional[torch.Tensor], dloss: Optional[torch.Tensor]):
        from .llama_train import llama_backward
        if ctx.saved is None:
            raise _spent("SetokimLlamaPrefill.forward")
        saved, ctx.saved = ctx.saved, None
        (logits, labels, attention_mask, loss_out), ctx.lm = ctx.lm, None
        like, ctx.like = ctx.like, None
        if not ctx.needs_input_grad[1] or (dlogits is None and (dloss is None or loss_out is None)):
            return None, None, None, None, None
        B, T, V = logits.shape
        w = ctx.prefill.lm_head.weight.detach().contiguous()
        gran = ops.k_align(logits.dtype)
        Vp = ops.round_up(V, gran)                                    # the dX GEMM contracts over the vocabulary: zero columns up to its granule
        dl = (torch.zeros if Vp != V else torch.empty)((B * T, Vp), dtype=logits.dtype, device=logits.device)
        view = dl[:, :V].view(B, T, V) if Vp == V else dl.view(B, T, Vp)[:, :, :V]
        if dloss is not None and loss_out is not None:
            ops.lm_loss_bwd(logits, labels, attention_mask, loss_out, upstream=dloss, out=view)
            if dlogits is not None:
                view += dlogits.to(logits.dtype)
        else:
            view.copy_(dlogits.to(logits.dtype))
        del logits
        dhidden = ops.linear(dl, ops.transpose(w, pad_to=gran))     # lm_head dX
        del dl
        dx = llama_backward(ctx.prefill.model, saved, dhidden.reshape(B, T, -1))
        return None, _grad_as(dx, like), None, None, None


# ----------------------------------------------------------------------------------------------------------------------------
# the frozen LLM with LoRA adapters (lora.py): the reference's finetune stage trains the adapters (and the projector) through the same loss
# ----------------------------------------------------------------------------------------------------------------------------
def _adapter_grads(model, grads: Dict[str, torch.Tensor], params: Sequence[torch.Tensor], needs: Sequence[bool]):
    """The fp32 gradients of llama_lora_backward in the order of LoraAdapters.flat(), each in its adapter's dtype; None where none is wanted."""
    names, _ = model.lora.flat()
    return tuple(_grad_as(grads[n], p) if need else None for n, p, need in zip(names, params, needs))


class LlamaLoraFn(torch.autograd.Function):
    """hidden = LlamaModel(inputs_embeds) with adapters attached and the stack frozen: d / d inputs_embeds and every dA, dB.
    `params`: LoraAdapters.flat()'s tensors, passed so that autograd routes their gradients."""

    @staticmethod
    def forward(ctx, model, inputs_embeds: torch.Tensor, attention_mask, position_ids, *params: torch.Tensor):
        from .llama_train import llama_lora_forward_train
        hidden, saved = llama_lora_forward_train(model, inputs_embeds.detach(), attention_mask, position_ids)
        ctx.model, ctx.saved, ctx.like, ctx.params = model, saved, inputs_embeds, params
        return hidden

    @staticmethod
    def backward(ctx, dhidden: torch.Tensor):
        from .llama_train import llama_lora_backward
        if ctx.saved is None:
            raise _spent("LlamaModel.forward")
        saved, ctx.saved = ctx.saved, None
        like, ctx.like = ctx.like, None
        dx, grads = llama_lora_backward(ctx.model, saved, dhidden)
        out = _adapter_grads(ctx.model, grads, ctx.params, ctx.needs_input_grad[4:])
        return (None, _grad_as(dx, like) if ctx.needs_input_grad[1] else None, None, None) + out


class LlamaLoraLMFn(torch.autograd.Function):
    """LlamaLMFn with adapters attached: (logits, loss) and, backward, d / d inputs_embeds plus every dA, dB."""

    @staticmethod
    def forward(ctx, prefill, inputs_embeds: torch.Tensor, attention_mask, position_ids, labels, *params: torch.Tensor):
        from .llama_train import llama_lora_forward_train
        hidden, saved = llama_lora_forward_train(prefill.model, inputs_embeds.detach(), attention_mask, position_ids)
        B, T, D = hidden.shape
        w = prefill.lm_head.weight.detach().contiguous()
        logits = ops.linear(hidden.reshape(B * T, D), w).reshape(B, T, -1)
        loss_out = ops.lm_loss(logits, labels, attention_mask) if labels is not None else None
        ctx.prefill, ctx.saved, ctx.like, ctx.params = prefill, saved, inputs_embeds, params
        ctx.lm = (logits, labels, attention_mask, loss_out)
        ctx.set_materialize_grads(False)
        return logits, (loss_out[0].clone() if loss_out is not None else logits.new_zeros((), dtype=torch.float32))

    @staticmethod
    def backward(ctx, dlogits: Optional[torch.Tensor], dloss: Optional[torch.Tensor]):
        from .llama_train import llama_lora_backward
        if ctx.saved is None:
            raise _spent("SetokimLlamaPrefill.forward")
        saved, ctx.saved = ctx.saved, None
        (logits, labels, attention_mask, loss_out), ctx.lm = ctx.lm, None
        like, ctx.like = ctx.like, None
        none = (None,) * (5 + len(ctx.params))
        if dlogits is None and (dloss is None or loss_out is None):
            return none
        B, T, V = logits.shape
        w = ctx.prefill.lm_head.weight.detach().contiguous()
        gran = ops.k_align(logits.dtype)
        Vp = ops.round_up(V, gran)                                    # (as LlamaLMFn: the dX GEMM contracts over the vocabulary)
        dl = (torch.zeros if Vp != V else torch.empty)((B * T, Vp), dtype=logits.dtype, device=logits.device)
        view = dl[:, :V].view(B, T, V) if Vp == V else dl.view(B, T, Vp)[:, :, :V]
        if dloss is not None and loss_out is not None:
            ops.lm_loss_bwd(logits, labels, attention_mask, loss_out, upstream=dloss, out=view)
            if dlogits is not None:
                view += dlogits.to(logits.dtype)
        else:
            view.copy_(dlogits.to(logits.dtype))
        del logits
        dhidden = ops.linear(dl, ops.transpose(w, pad_to=gran))       # lm_head dX
        del dl
        dx, grads = llama_lora_backward(ctx.prefill.model, saved, dhidden.reshape(B, T, -1))
        out = _adapter_grads(ctx.prefill.model, grads, ctx.params, ctx.needs_input_grad[5:])
        return (None, _grad_as(dx, like) if ctx.needs_input_grad[1] else None, None, None, None) + out
