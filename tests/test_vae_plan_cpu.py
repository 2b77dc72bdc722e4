"""What the VAE records, frozen: tests/golden/vae_plan_launches.json holds (kind, variant, shape) of every launch of the decode and encode
segments of the tiny VAE of tests/test_vae_gpu.py, at batch 1 and 2, as recorded before the mid-block attention's per-image loop moved into
AutoencoderKL._attend.  Recorded again here on the CPU (nothing is launched) and compared: the plans did not change with the move."""
import json
import os

import pytest

from blobctrl_amd import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vae_plan_launches.json")


@pytest.fixture(scope="module")
def tiny_vae_cpu():
    from blobctrl_amd.vae import AutoencoderKL
    mp = pytest.MonkeyPatch()
    mp.setattr(AutoencoderKL, "_need_gpu", lambda self: None)          # (recording needs no device; running the plan would)
    sd = synth.synth_state_dict(synth.vae_param_shapes((32, 32, 64, 64), 2, 4), 21)
    yield AutoencoderKL(sd, norm_num_groups=8, device="cpu")
    mp.undo()


def _launches(seg):
    return [[m["kind"], m["variant"], list(m["shape"]) if m.get("shape") is not None else None] for m in seg.meta]


@pytest.mark.parametrize("B", [1, 2])
def test_the_vae_segments_record_the_frozen_launches(tiny_vae_cpu, B):
    frozen = json.load(open(GOLD))
    dec = _launches(tiny_vae_cpu._plan_decode(B, 8, 8).seg)
    enc = _launches(tiny_vae_cpu._plan_encode(B, 64, 64).seg)
    assert dec == frozen[f"decode-B{B}-8x8"] and enc == frozen[f"encode-B{B}-64x64"]
    # the mid-block attention: per image Q K^T, softmax, P V
    for launches in (dec, enc):
        at = [i for i, l in enumerate(launches) if l[0] == "vae_attn"]
        assert len(at) == 2 * B and all(launches[i + 1][0] == "softmax" for i in at[::2]) and at[1::2] == [i + 2 for i in at[::2]]
