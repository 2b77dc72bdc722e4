"""The packers of the folded 1x1 shortcut (BcGemm.S, csrc/conv_wreg.hip): `weights.pack_conv_wreg(w, wsc)` against the library's own index
map run on the CPU (`bc_conv_wreg_pack_host`, the function the device kernel `bc_conv_wreg_pack_sc` calls per lane slot), byte for byte, and
the 3x3-only form against the packer as it was before the fold existed (kept here as `_pack_3x3_only`)."""
import ctypes as C

import pytest
import torch

from blobctrl_amd import _lib
from blobctrl_amd.weights import WREG_TILES, pack_conv_wreg

SHAPES = [(320, 320, 640), (640, 640, 1920), (1280, 1280, 2560), (320, 320, 960), (640, 320, 320), (160, 64, 64)]


def _pack_3x3_only(w):
    """pack_conv_wreg of the commit before the shortcut fold, verbatim."""
    N, K = w.shape
    Cin = K // 9
    nch = Cin // 64
    v = w.reshape(N // 160, 10, 16, 3, 3, nch, 2, 4, 8)
    parts = []
    for blk in range(N // 160):
        for t0, nt in WREG_TILES:
            g = v[blk, t0:t0 + nt]
            g = g.permute(5, 4, 3, 2, 0, 6, 1, 7)
            parts.append(g.reshape(-1))
    return torch.cat(parts).reshape(N, K)


def _weights(N, Cin, Cs, seed=0):
    g = torch.Generator().manual_seed(seed)
    # distinct 16-bit patterns wherever possible: a misplaced fragment cannot hide behind equal values
    w = torch.randint(-32768, 32767, (N, 9 * Cin), generator=g, dtype=torch.int16)
    ws = torch.randint(-32768, 32767, (N, Cs), generator=g, dtype=torch.int16) if Cs else None
    return w, ws


def _host_pack(w, ws):
    lib = _lib.load()
    N, K = w.shape
    Cs = ws.shape[1] if ws is not None else 0
    out = torch.empty(N, K + Cs, dtype=torch.int16)
    rc = lib.bc_conv_wreg_pack_host(w.data_ptr(), N, K // 9, ws.data_ptr() if ws is not None else None, Cs, out.data_ptr())
    assert rc == 0
    return out


@pytest.mark.parametrize("N,Cin,Cs", SHAPES)
def test_folded_pack_matches_library(N, Cin, Cs):
    w, ws = _weights(N, Cin, Cs)
    got, ref = pack_conv_wreg(w, ws), _host_pack(w, ws)
    assert got.shape == (N, 9 * Cin + Cs) and torch.equal(got.contiguous(), ref)


@pytest.mark.parametrize("N,Cin", [(320, 320), (640, 640), (1280, 1280), (320, 64)])
def test_unfolded_pack_is_unchanged(N, Cin):
    w, _ = _weights(N, Cin, 0, seed=1)
    old = _pack_3x3_only(w)
    assert torch.equal(pack_conv_wreg(w).contiguous(), old) and torch.equal(_host_pack(w, None), old)


def test_folded_stream_layout():
    """What the kernel assumes: wave stream (block, group, K half) = its nine-tap fragments in the 3x3-only order, then per shortcut chunk
    NT fragments, lane l holding wsc[n0 + 16 tile + (l & 15)][64 chunk + 32 kg + 8 (l >> 4) .. + 8]."""
    N, Cin, Cs = 320, 128, 192
    w, ws = _weights(N, Cin, Cs, seed=2)
    full, plain = pack_conv_wreg(w, ws).reshape(-1), _pack_3x3_only(w).reshape(-1)
    nch, nsc = Cin // 64, Cs // 64
    pos = pos3 = 0
    for blk in range(N // 160):
        for t0, nt in WREG_TILES:
            for kg in range(2):
                n3 = nch * 9 * nt * 512
                assert torch.equal(full[pos:pos + n3], plain[pos3:pos3 + n3])
                pos, pos3 = pos + n3, pos3 + n3
                frag = full[pos:pos + nsc * nt * 512].reshape(nsc, nt, 64, 8)
                for c in range(nsc):
                    for t in range(nt):
                        for lane in (0, 17, 63):
                            n, k = blk * 160 + (t0 + t) * 16 + (lane & 15), c * 64 + kg * 32 + 8 * (lane >> 4)
                            assert torch.equal(frag[c, t, lane], ws[n, k:k + 8])
                pos += nsc * nt * 512
    assert pos == full.numel() and pos3 == plain.numel()


def test_struct_mirror_and_eligibility():
    lib = _lib.load()
    assert lib.bc_sizeof_gemm() == C.sizeof(_lib.BcGemm)
    assert lib.bc_conv_wreg_sc_eligible(1280, 1280, 16, 32, 2560, 1280, 0) == 1
    assert lib.bc_conv_wreg_sc_eligible(320, 320, 64, 128, 640, 0, 0) == 1
    assert lib.bc_conv_wreg_sc_eligible(320, 320, 64, 128, 600, 0, 0) == 0      # Cs % 64
    assert lib.bc_conv_wreg_sc_eligible(320, 320, 64, 128, 640, 96, 0) == 0     # split point % 64
    assert lib.bc_conv_wreg_sc_eligible(320, 320, 4, 4, 640, 0, 0) == 0         # the map is too small for the kernel's tile
