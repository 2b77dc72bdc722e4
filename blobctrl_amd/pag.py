"""Perturbed-attention guidance (PAG, https://arxiv.org/abs/2403.17377) on the host: which self-attentions a layer id names, and the
guidance scale of every step.

Restated reference code (D/ = diffusers/src/diffusers/): D/pipelines/pag/pag_utils.py PAGMixin - `_set_pag_attn_processor` (the matching
rule), `set_pag_applied_layers` (the type check), `_get_pag_scale` (the adaptive scale).  What the matched layers then compute is the
planner's (engine.TrunkPlan.self_attention) and the step's (csrc/pag.hip)."""
import re
from typing import List, Sequence, Tuple, Union


def normalize_layers(pag_applied_layers: Union[str, List[str]]) -> List[str]:
    """`set_pag_applied_layers`: a string or a list of strings; anything else is a ValueError, in the reference's words."""
    if not isinstance(pag_applied_layers, list):
        pag_applied_layers = [pag_applied_layers]
    for layer in pag_applied_layers:
        if not isinstance(layer, str):
            raise ValueError(f"Expected either a string or a list of string but got type {type(layer)}")
    return list(pag_applied_layers)


def self_attention_names(unet_config) -> List[str]:
    """The names of the UNet's self-attention modules (`attn1` of every transformer block) in `named_modules` order - down blocks, up
    blocks, mid block, as UNet2DConditionModel registers them - from the trunk configuration: every down block but the last and every up
    block but the first hold one Transformer2DModel of one block per resnet (the SD-1.5 topology engine.record_forward runs)."""
    nb, lpb = len(unet_config.block_out_channels), unet_config.layers_per_block
    name = "{}.attentions.{}.transformer_blocks.0.attn1".format
    return [name(f"down_blocks.{i}", j) for i in range(nb - 1) for j in range(lpb)] + \
        [name(f"up_blocks.{i}", j) for i in range(1, nb) for j in range(lpb + 1)] + [name("mid_block", 0)]


def _is_fake_integral_match(layer_id: str, name: str) -> bool:
    layer_id, name = layer_id.split(".")[-1], name.split(".")[-1]
    return layer_id.isnumeric() and name.isnumeric() and layer_id == name


def matched_names(unet_config, layer_id: str) -> List[str]:
    """The self-attention modules one layer id names: `re.search(layer_id, name)` over the module names, without the "fake integral
    matches"; ValueError when there is none."""
    names = [n for n in self_attention_names(unet_config) if re.search(layer_id, n) is not None and not _is_fake_integral_match(layer_id, n)]
    if not names:
        raise ValueError(f"Cannot find PAG layer to set attention processor for: {layer_id}")
    return names


def resolve_layers(unet_config, ids: Union[str, Sequence[str]]) -> Tuple[str, ...]:
    """Layer ids -> the sorted tuple of block prefixes ("mid_block.attentions.0.", ...) the planner perturbs: what a plan key holds."""
    found = set()
    for layer_id in normalize_layers(list(ids) if isinstance(ids, tuple) else ids):
        found.update(n[: -len("transformer_blocks.0.attn1")] for n in matched_names(unet_config, layer_id))
    return tuple(sorted(found))


def pag_scale_at(t, pag_scale: float, pag_adaptive_scale: float = 0.0) -> float:
    """`_get_pag_scale(t)`: pag_scale, or with pag_adaptive_scale > 0 max(0, pag_scale - pag_adaptive_scale * (1000 - t)).  The reference
    evaluates this on the scheduler's timestep TENSOR with Python scalars - float32 arithmetic, for integer and for float32 (Euler)
    timesteps alike - so it is float32 arithmetic here, and the value is the reference's bit for bit."""
    if pag_adaptive_scale > 0:
        import torch
        tt = torch.as_tensor(t)
        tt = tt.to(torch.float32) if tt.is_floating_point() else tt
        return max(0.0, float(float(pag_scale) - float(pag_adaptive_scale) * (1000 - tt)))
    return float(pag_scale)


def pag_table(timesteps, pag_scale: float, pag_adaptive_scale: float = 0.0) -> List[float]:
    """The scale of every network evaluation of an edit (a Heun table: one row per evaluation, like `coef`): the contents of a PAG plan's
    `pag_table` buffer."""
    return [pag_scale_at(t, pag_scale, pag_adaptive_scale) for t in timesteps]


def is_active(pag_scale, pag_applied_layers) -> bool:
    """`do_perturbed_attention_guidance`: pag_scale > 0 and at least one applied layer."""
    return pag_scale > 0 and pag_applied_layers is not None and len(pag_applied_layers) > 0
