"""Inputs, fp64 truths and input conditions shared by tests/test_gpu_groups.py (which checks the decode kernels against
them) and tests/test_host_groups.py (which checks the conditions on the CPU).  Not a test module.

Everything is drawn on the CPU from one seeded generator and then moved to `device`, so both files see the same numbers.
The truths are those of attn_ref.attention_fp64 on the cache as it stands after the append (dequantised for
the e4m3 kinds, the NaN padding zeroed: it is masked); the only arithmetic added here is the signed distance pos - j that
the "keys right of the query matter" condition swaps in for attn_ref.distance's |pos - j|."""
from types import SimpleNamespace

import torch

import attn_ref as ar
from test_gpu_alibi import BIAS_MATTERS
from test_gpu_sink import REF_MATTERS
from test_gpu_softcap import CAP_MATTERS, _amp

F16, BF16 = torch.float16, torch.bfloat16
KINDS = ("plain", "softcap", "alibi", "sink", "fp8", "fp8_sink")
# (H, H_kv, S_q): the g * S_q (query, head) rows of a K/V head are cut into 32-row blocks
GEOMS = [
    (6, 2, 11),    # g = 3, 33 rows: the second block holds one row, the boundary 32 cuts query 10's heads
    (14, 2, 10),   # g = 7, 70 rows: boundaries 32 and 64, both inside a query
    (5, 1, 13),    # g = 5, MQA, 65 rows: a one-row tail block
    (24, 2, 3),    # g = 12, 36 rows
    (8, 2, 16),    # g = 4, 64 rows: aligned boundaries, the first multi-block run of the variants
    (2, 2, 40),    # g = 1: rows are queries, the blocks' key ranges differ most
]
B, S_CACHE = 6, 704
FILL = [0, 1, 31, 33, 300, 650]                       # before the append: L = 0, L < S_q, either side of a 32-key tile
WINDOWS = [(-1, -1), (-1, 0), (5, 0), (40, 8), (0, 0)]
SPLITS = (0, 1, 3, 7)
# the chosen parameters (test_host_groups.py checks on the CPU that each transform matters with them)
CAP = 30.0                       # Q drawn at _amp(CAP, scale, D): score std 0.6 CAP
SINK_LO, SINK_HI = 0.0, 8.0      # sinks = linspace over the heads
SLOPE_LO, SLOPE_HI = 0.15, 1.0   # steep: at most S_q - 1 keys lie right of a query, and they have to matter
SLOPE_STEP = 11                  # head h takes step (11 h + 2) mod H of H: neighbouring heads get distant slopes
V_GAIN = 1.7                     # the e4m3 kinds quantise V * 1.7 (test_gpu_kvcache_fp8.py)


def geom_id(geom):
    return "h%dkv%dq%d" % geom


def row_blocks(geom):
    H, Hkv, Sq = geom
    return -(-(H // Hkv) * Sq // 32)


def s_new(gi, dtype, D):
    """k_new / v_new rows appended: 2 on every second parametrisation, 0 otherwise."""
    return 2 * ((gi + (dtype == BF16) + (D == 128)) % 2)


def sinks_of(H):
    return torch.linspace(SINK_LO, SINK_HI, H, dtype=torch.float32)


def slopes_of(H):
    """(B, H) fp32, every entry distinct: head h at step (11 h + 2) mod H between SLOPE_LO and SLOPE_HI, sequence b
    times 1 + 0.07 b."""
    step = (SLOPE_STEP * torch.arange(H) + 2) % H
    base = SLOPE_LO + (SLOPE_HI - SLOPE_LO) * step.float() / H
    s = (base[None, :] * (1.0 + 0.07 * torch.arange(B).float())[:, None]).contiguous()
    assert s.flatten().unique().numel() == B * H
    return s


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16}[t.element_size()])


def make_case(kind, geom, dtype, D, snew, device):
    """The inputs of one decode call, the cache it must leave behind (bits) and that cache in fp64."""
    import My_FlashAttention_optimized as M
    H, Hkv, Sq = geom
    fp8 = kind.startswith("fp8")
    scale = D ** -0.5
    g = torch.Generator().manual_seed(1000 * H + 10 * Sq + D + snew)
    q = torch.randn(B, H, Sq, D, generator=g)
    if kind == "softcap":
        q = q * _amp(CAP, scale, D)
    q = q.to(dtype)
    kf, vf = (torch.randn(B, Hkv, S_CACHE, D, generator=g) for _ in range(2))
    kn, vn = (torch.randn(B, Hkv, max(snew, 1), D, generator=g).to(dtype) for _ in range(2))
    kd = vd = None
    if fp8:
        kc, kd = M.quantize_kv_fp8(kf)
        vc, vd = M.quantize_kv_fp8(vf * V_GAIN)
    else:
        kc, vc = kf.to(dtype), vf.to(dtype)
    ka, va = kc.clone(), vc.clone()
    # the rows the append must write: k_new / v_new themselves, or their e4m3 bytes under the cache's descales
    kq, vq = (M.quantize_kv_fp8(kn, kd)[0], M.quantize_kv_fp8(vn, vd)[0]) if fp8 else (kn, vn)
    for b, L in enumerate(FILL):   # NaN (0x7F) past the fill level; the appended rows overwrite their part of it
        for t in (kc, vc, ka, va):
            _bits(t)[b, :, L:] = 0x7F if fp8 else 0x7FFF
        if snew:
            _bits(ka)[b, :, L:L + snew] = _bits(kq)[b]
            _bits(va)[b, :, L:L + snew] = _bits(vq)[b]
    if not snew:
        kn = vn = None
    deq = lambda x, d: torch.nan_to_num(x.double() * (d.double().reshape(-1, Hkv, 1, 1) if d is not None else 1.0), nan=0.0)
    c = SimpleNamespace(kind=kind, geom=geom, dtype=dtype, D=D, scale=scale, snew=snew, Ls=[L + snew for L in FILL],
                        q=q, kc=kc, vc=vc, kn=kn, vn=vn, kd=kd, vd=vd, k_after=ka, v_after=va, kr=deq(ka, kd), vr=deq(va, vd),
                        sl=torch.tensor(FILL, dtype=torch.int32), slopes=slopes_of(H), sinks=sinks_of(H))
    for n, t in list(vars(c).items()):
        if isinstance(t, torch.Tensor):
            setattr(c, n, t.to(device))
    assert all(0 <= L <= S_CACHE for L in c.Ls)
    return c


def masks(c, window):
    """vis [B, 1, S_q, S_c] bool and the signed distance pos - j [B, 1, S_q, S_c] fp64 (bottom-right aligned)."""
    Sq, dev = c.geom[2], c.q.device
    vis = torch.stack([ar.visible(Sq, S_CACHE, window[0], window[1], dev, L=L) for L in c.Ls])[:, None]
    i = torch.arange(Sq, device=dev, dtype=torch.float64)[:, None]
    j = torch.arange(S_CACHE, device=dev, dtype=torch.float64)[None, :]
    signed = torch.stack([(i + (L - Sq)) - j for L in c.Ls])[:, None]
    dist = torch.stack([ar.distance(Sq, S_CACHE, dev, L=L) for L in c.Ls])[:, None]
    assert torch.equal(dist, signed.abs())
    return vis, dist, signed


def truth(c, window):
    """fp64 O / LSE / SABS of the call (`gt`), O without the transform (`base`, None for plain and fp8), for ALiBi also O
    with the signed distance (`signed`) and whether a visible key lies right of its query (`right`); vis and the keyless
    rows [B, H, S_q]."""
    vis, dist, signed = masks(c, window)
    a = (c.q, c.kr, c.vr, None, c.scale, vis)
    kw = {"softcap": dict(cap=CAP), "alibi": dict(slopes=c.slopes, dist=dist), "sink": dict(sinks=c.sinks),
          "fp8_sink": dict(sinks=c.sinks)}.get(c.kind, {})
    out = SimpleNamespace(vis=vis, gt=ar.attention_fp64(*a, **kw), base=None, signed=None, right=None)
    if kw:
        out.base = ar.attention_fp64(*a)["O"]
    if c.kind == "alibi":
        out.signed = ar.attention_fp64(*a, slopes=c.slopes, dist=signed)["O"]
        out.right = bool((vis & (signed < 0)).any())
    out.nokey = ~vis.expand(B, c.geom[0], c.geom[2], S_CACHE).any(-1)
    return out


def _far(pairs):
    num = sum(float((a - b).square().sum()) for a, b in pairs)
    den = sum(float(a.square().sum()) for a, b in pairs)
    return (num / den) ** 0.5


MATTERS = {"softcap": CAP_MATTERS, "alibi": BIAS_MATTERS, "sink": REF_MATTERS, "fp8_sink": REF_MATTERS}


def check_conditions(c, truths):
    """The conditions on the reference, before any kernel output is looked at: the transform moves the fp64 O by at least
    its file's threshold over the windows other than (0, 0) (where P = 1 whatever the bias), and for ALiBi some visible key
    lies right of its query and that side moves O by BIAS_MATTERS on the (-1, -1) and (40, 8) windows.  Returns the figures."""
    fig = {}
    if c.kind in MATTERS:
        fig["matters"] = _far([(truths[w].gt["O"], truths[w].base) for w in WINDOWS if w != (0, 0)])
        assert fig["matters"] >= MATTERS[c.kind], (c.kind, c.geom, "the transform moves the fp64 O by %.3e only" % fig["matters"])
    if c.kind == "alibi":
        for w in ((-1, -1), (40, 8)):
            assert truths[w].right, (c.geom, w, "no visible key right of a query")
            fig["right(%d,%d)" % w] = _far([(truths[w].gt["O"], truths[w].signed)])
            assert fig["right(%d,%d)" % w] >= BIAS_MATTERS, (c.geom, w, "the keys right of the queries move O by %.3e only" % fig["right(%d,%d)" % w])
    return fig
