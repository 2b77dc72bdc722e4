"""Helpers shared by the `-m gpu` tests (everything here goes through the C ABI of libblobctrl_hip.so)."""
import ctypes as C

import torch

from blobctrl_amd.engine import TrunkConfig
from tests.common import TINY


def tiny_trunk_configs():
    c = TINY
    u = TrunkConfig(in_channels=5, block_out_channels=c["boc"], num_heads=c["heads"], norm_num_groups=c["groups"],
                    cross_attention_dim=c["ctx"], out_channels=4, is_blobnet=False)
    b = TrunkConfig(in_channels=4 + 1 + c["feat"], block_out_channels=c["boc"], num_heads=c["heads"],
                    norm_num_groups=c["groups"], cross_attention_dim=None, out_channels=0, is_blobnet=True)
    return u, b


def make_pipeline(usd, bsd, scheduler="unipc", use_graphs=True):
    from blobctrl_amd.pipeline import BlobCtrlEngine
    u, b = tiny_trunk_configs()
    return BlobCtrlEngine(usd, bsd, u, b, device="cuda:0", scheduler=scheduler, use_graphs=use_graphs)


def launch_step(lib, form, eps, latents, coef, idx, hist, guidance, B, h, w, eps_out, advance=1, noise=None, nsteps=0):
    """One CFG + scheduler step through ctypes on the current stream; `form` "step" | "noise" | "step3" names the entry point
    (bc_cfg_scheduler_step / _step_noise / _step3), `noise` / `nsteps` are the arguments only the latter two take.  Returns the C
    return code without synchronising."""
    if form == "step":
        name, extra = "bc_cfg_scheduler_step", ()
    elif form == "noise":
        name, extra = "bc_cfg_scheduler_step_noise", (noise.data_ptr(), nsteps)
    else:
        assert form == "step3", form
        name, extra = "bc_cfg_scheduler_step3", (nsteps,)
    return getattr(lib, name)(eps.data_ptr(), latents.data_ptr(), coef.data_ptr(), idx.data_ptr(), hist.data_ptr(), guidance, B, h, w,
                              *extra, eps_out.data_ptr(), advance, C.c_void_p(torch.cuda.current_stream().cuda_stream))
