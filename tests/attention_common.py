"""Inputs and float64 references for the attention kernel tests (tests/test_attention_gpu.py, tests/test_attention_cpu.py).

With Gaussian inputs at Nkv >= 1000 one key carries ~1e-3 of a query's mass and |ref| stays below 0.3, so the project's attention bar
(3e-3 + 2e-3 |ref|) cannot see a key that leaks past the ragged-tail mask or one that is dropped.  The inputs here are built
so that one key is worth many bars, and `key_set_power` / `causal_power` prove it FROM THE REFERENCE ALONE: they return how far (in bars) a
float64 reference with a perturbed key set lies from the true one.  Everything runs on whatever device the tensors are on."""
import math

import numpy as np
import torch

from tests.common import g

BAR_ATOL, BAR_RTOL = 3e-3, 2e-3         # the attention bar of tests/test_kernels_gpu.py::test_attention
POWER = 20.0                            # a perturbed key set must move the reference by this many bars somewhere
SCORE_LIMIT = 25.0                      # the scale rides in the fp16 query: the documented range of a score


def sign_vector(d, heads):
    u = torch.from_numpy(np.random.Generator(np.random.PCG64(1234 + d)).integers(0, 2, size=d).astype(np.float32) * 2 - 1)
    return u.repeat(heads)


def last_tile_key(Nkv):
    return (Nkv - 1) // 64 * 64


LEAK_AMP = 0.7


def make_inputs(kind, B, heads, d, Nq, Nkv, seed=0):
    """fp16 q [B][Nq][C], k [B][Nkv][C], v [B][Nkv][C] on the CPU.  `plain`: Gaussian.  `leak`: every valid score shifted to about -10, so a
    key with score 0 (a zero K row behind the mask) would take most of a query's mass.  `drop`: keys 0, the first key of the last 64-key
    tile and Nkv - 1 score about +8 for every third query, so each of them carries a large share of those queries' mass."""
    Cc = heads * d
    q, k, v = g(seed + 1, B, Nq, Cc), g(seed + 2, B, Nkv, Cc), g(seed + 3, B, Nkv, Cc)
    u, t = sign_vector(d, heads), math.sqrt(10.0 / math.sqrt(d))
    if kind == "leak":
        q, k = LEAK_AMP * q, LEAK_AMP * k            # (at d = 8 products of unit Gaussians have tails that would pass SCORE_LIMIT)
        q += t * u
        k -= t * u
    elif kind == "drop":
        q[:, ::3] += t * u
        for j in (0, last_tile_key(Nkv), Nkv - 1):
            k[:, j] = 0.8 * t * u
    else:
        assert kind == "plain", kind
    return q.half(), k.half(), v.half()


RAMP_STEP, RAMP_SPAN, RAMP_NOISE = 0.5, 16.0, 0.5


def make_ramp_inputs(B, heads, d, N, seed=0):
    """Causal inputs: the score of key j rises linearly with j (RAMP_STEP per key, total span <= RAMP_SPAN) under Gaussian noise of std
    RAMP_NOISE, so the newest visible key - the one on the diagonal - is the heaviest of every query."""
    Cc = heads * d
    u, t = sign_vector(d, heads), math.sqrt(10.0 / math.sqrt(d))
    step = min(RAMP_STEP, RAMP_SPAN / max(N - 1, 1))
    ramp = (torch.arange(N, dtype=torch.float32) - (N - 1) / 2) * step            # centred: |ramp| <= RAMP_SPAN / 2
    q = RAMP_NOISE * g(seed + 1, B, N, Cc) + t * u
    k = g(seed + 2, B, N, Cc) + (ramp / 10.0)[None, :, None] * (t * u)           # (t u) . (t u) / sqrt(d) = 10
    return q.half(), k.half(), g(seed + 3, B, N, Cc).half()



def _heads_view(x, heads, d):
    return x.double().view(x.shape[0], heads, d).transpose(0, 1)                 # [N][C] -> [heads][N][d]


def scores(q, k, heads, d, scale):
    """float64 scale * Q K^T of one image: [heads][Nq][Nkv]."""
    return _heads_view(q, heads, d) @ _heads_view(k, heads, d).transpose(1, 2) * scale


def _attend(s, vh):
    return (torch.softmax(s, -1) @ vh).transpose(0, 1).reshape(s.shape[1], -1)  # [Nq][C]


def reference(q, k, v, heads, d, scale, causal=False):
    """softmax(scale Q K^T) V in float64 from the fp16-rounded inputs, one image at a time -> [B][Nq][C] float64."""
    out = []
    for b in range(q.shape[0]):
        s = scores(q[b], k[b], heads, d, scale)
        if causal:
            s = s + torch.full(s.shape[1:], float("-inf"), dtype=s.dtype, device=s.device).triu(1)
        out.append(_attend(s, _heads_view(v[b], heads, d)))
    return torch.stack(out)


def bar(ref):
    return BAR_ATOL + BAR_RTOL * ref.abs()


def worst(out, ref):
    """(max err / bar, (b, head, query, column)) of an output against its float64 reference; `d` columns per head."""
    r = (out.double() - ref).abs() / bar(ref)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))      # a NaN output is the worst error there is
    i = int(r.argmax())
    return float(r.flatten()[i]), np.unravel_index(i, r.shape)


def assert_within_bar(out, ref, d, what):
    w, (b, qi, c) = worst(out, ref)
    print(f"{what}: worst err/bar {w:.3f} at (b={b}, head={c // d}, query={qi}, column={c % d})")
    assert w <= 1.0, f"{what}: worst err/bar {w:.2f} at (b={b}, head={c // d}, query={qi}, column={c % d})"


def key_set_power(q, k, v, heads, d, scale):
    """How many bars the float64 reference moves (max over elements) when the key set is wrong by one key: {'extra': one appended zero key
    with a zero V row, 'last': key Nkv-1 removed, 'first': key 0 removed, 'tile': the first key of the last tile removed}.  Removing the
    only key leaves nothing to attend to: that entry is then absent.  Also returns the largest |score|."""
    Nkv = k.shape[1]
    power, smax = {}, 0.0
    for b in range(q.shape[0]):
        s, vh = scores(q[b], k[b], heads, d, scale), _heads_view(v[b], heads, d)
        smax = max(smax, float(s.abs().max()))
        ref = _attend(s, vh)
        bars = bar(ref)
        variants = {"extra": _attend(torch.cat([s, torch.zeros_like(s[..., :1])], -1), torch.cat([vh, torch.zeros_like(vh[:, :1])], 1))}
        if Nkv > 1:
            for name, j in (("last", Nkv - 1), ("first", 0), ("tile", last_tile_key(Nkv))):
                sj = s.clone()
                sj[..., j] = float("-inf")
                variants[name] = _attend(sj, vh)
        for name, o in variants.items():
            power[name] = max(power.get(name, 0.0), float(((o - ref).abs() / bars).max()))
    return power, smax


def _block_min(r):
    """min over 32-query blocks of the block's max: r [Nq][C]."""
    return min(float(r[i:i + 32].max()) for i in range(0, r.shape[0], 32))


def causal_power(q, k, v, heads, d, scale):
    """The same for the causal mask: {'admit': key i+1 visible to query i, 'hide': key i hidden from query i (queries >= 1)}.  The early
    queries see few keys and move by hundreds of bars whatever the inputs, so the figure is the WEAKEST 32-query block's largest move: a
    wrong mask is visible at every depth of the sequence, not only at its start."""
    N = q.shape[1]
    power, smax = {"admit": float("inf"), "hide": float("inf")}, 0.0
    for b in range(q.shape[0]):
        s, vh = scores(q[b], k[b], heads, d, scale), _heads_view(v[b], heads, d)
        smax = max(smax, float(s.abs().max()))
        ninf = torch.full(s.shape[1:], float("-inf"), dtype=s.dtype, device=s.device)
        ref = _attend(s + ninf.triu(1), vh)
        bars = bar(ref)
        if N > 1:
            adm = (_attend(s + ninf.triu(2), vh) - ref).abs() / bars
            power["admit"] = min(power["admit"], _block_min(adm[:-1]))             # the last query has no key i+1
            hid = _attend((s + ninf.triu(0))[:, 1:], vh)                           # query 0 would have no key left
            power["hide"] = min(power["hide"], _block_min((hid - ref[1:]).abs() / bars[1:]))
    return power, smax


# the loop's real attention launches: (d, B, heads, Nq, Nkv, causal) -> build (NW * 10 + WPE), for tests/test_attention_cpu.py
LOOP_SHAPES = [
    ((40, 1, 8, 8192, 8192, 0), 84), ((40, 2, 8, 8192, 8192, 0), 84),          # 64 x 128 level, BlobNet (batch 1) and UNet (CFG pair)
    ((80, 1, 8, 2048, 2048, 0), 81), ((80, 2, 8, 2048, 2048, 0), 81),          # 32 x 64 level
    ((160, 1, 8, 512, 512, 0), 41), ((160, 2, 8, 512, 512, 0), 41),            # 16 x 32 level
    ((160, 2, 8, 128, 128, 0), 41),                                            # mid block, 8 x 16
    ((40, 2, 8, 8192, 77, 0), 41), ((80, 2, 8, 2048, 77, 0), 41), ((160, 2, 8, 512, 77, 0), 41), ((160, 2, 8, 128, 77, 0), 41),   # cross
    ((64, 2, 12, 77, 77, 1), 41),                                              # CLIP text encoder, causal
    ((64, 1, 16, 257, 257, 0), 41),                                            # DINOv2
]
