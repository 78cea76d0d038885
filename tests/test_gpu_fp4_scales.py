"""GPU tests of the MXFP4 format's whole domain (include/mi355fa_kvcache_fp4.h, "Exactness" and "The quantiser"): every scale
byte 0..254 through the kernels' conversions, and the device quantiser at the extreme rows of the host suite.

tests/test_gpu_kvcache_fp4.py draws scale bytes from 121..133 and appends binades -8..8.  The quantiser writes 101..140 from
finite fp16 inputs and 0..252 from finite bf16 ones, and the header promises every product that q's dtype represents without
rounding.  Here:

  * element for element over every scale byte: one key per sequence and unit-vector queries (head h asks for element h), so
    that O is V itself and LSE is one score.  The blocks of a step carry every scale byte 0..254, twice, in two assignments
    (ascending, and scattered so that the blocks of a row lie binades apart), K and V with different bytes.  Each block holds
    every code that T represents at its scale, signs included, in an order of its own; what is left of a partial block is
    codes 0 and 8, so no element is unrepresentable and no 0 * inf enters a score.  That domain is computed from
    dequantize_kv_mxfp4 and held to the table written out below.  O equals the fp64 value of V exactly and has the bits of
    flash_attention_kvcache (the 16-bit kernel) on the cache dequantised to T -- the sign of a zero is that kernel's, +0, since
    attention adds -0 * p to +0 -- and LSE has that kernel's bits, at the same forced split count and softmax_scale = 2^-3
    (6 * 2^125 stays finite in log2 units).  With a single key and a one-hot query each score is one product plus zeros: the
    two kernels perform the same arithmetic whatever their summation order.  Padded and paged at D = 64 and 128, packed at
    D = 64, 128 and 256 (both halves of a D = 256 row carry extreme scales).
  * all-zero blocks (codes 0 and 8) under every scale byte 0..254 give zeros and a finite LSE.
  * the device quantiser (quant32_fp4, through the padded and the packed append) on test_host_kvcache_fp4.cases: amax at the
    largest finite value, at 1 and 3 smallest subnormals, around the smallest normal, all ties, saturation, signed zeros and
    the zero block.  The bytes written are quantize_kv_mxfp4's on the CPU and np_quantize's codes, bit for bit; and the
    round trip: the same call, one key per sequence, returns as O exactly dequantize_kv_mxfp4 of the appended V row.

e = 255, NaN and Inf, and (e, code) pairs T does not represent are not fed: the header leaves them unspecified.

Measured on an MI355X: every assertion holds, in both dtypes.  v_cvt_scalef32_pk_{f16,bf16}_fp4 reads the exponent field of
its scale operand alone, so e = 0 scales by 2^-127, and it delivers results that are subnormal in T; the header's Exactness
clause stands for every scale byte (csrc/fa_decode.hip's e8m0_scale comment, which said otherwise of e = 0, is corrected).
The module takes about 3 s (34 cases, each well below a second)."""
import numpy as np
import pytest
import torch

import raggedcheck as rg
import variantcheck as vck
import test_gpu_kvcache_fp4 as t4
import test_host_kvcache_fp4 as th
from test_gpu_kvcache_fp4 import BF16, DT, F16, FF, IDS

pytestmark = pytest.mark.gpu

MAGS = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)             # e2m1 codes 0..7; bit 3 is the sign
# the scale bytes at which T represents all 16 codes, and the magnitudes it represents at the bytes beside them (computed on
# the CPU; test_the_domain_is_the_one_written_out holds domain() to it).  Every other byte: zeros only.
FULL = {F16: range(104, 141), BF16: range(0, 253)}
PARTIAL = {F16: {101: (0.0, 4.0), 102: (0.0, 2.0, 4.0, 6.0), 103: (0.0, 1.0, 2.0, 3.0, 4.0, 6.0),
                 141: (0.0, 0.5, 1.0, 1.5, 2.0, 3.0), 142: (0.0, 0.5, 1.0, 1.5), 143: (0.0, 0.5)},
           BF16: {253: (0.0, 0.5, 1.0, 1.5, 2.0, 3.0), 254: (0.0, 0.5, 1.0, 1.5)}}
SCALE = 2.0 ** -3
CALLS = [("padded", 64), ("padded", 128), ("paged", 64), ("paged", 128), ("packed", 64), ("packed", 128), ("packed", 256)]
CALL_IDS = ["%s-d%d" % c for c in CALLS]
# (multiplier, offset) of the scale byte of block idx, for V and for K: ascending, and scattered (97 and 61 are coprime to 255)
ASSIGN = [((1, 0), (1, 128)), ((97, 31), (61, 7))]


def _F():
    import fp4_kvcache as F
    return F


def _R():
    import fp4_ragged_kvcache as R
    return R


def _M():
    import My_FlashAttention_optimized as M
    return M


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def value64(codes, e):
    """e2m1(code) * 2^(e - 127) in fp64, by another route than dequantize_kv_mxfp4: codes [..., n] with e [...] or [..., 1]"""
    lut = torch.tensor(MAGS + tuple(-m for m in MAGS), dtype=torch.float64)
    e = e.reshape(*e.shape, 1) if e.dim() < codes.dim() else e
    return lut[codes.long()] * torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double() - 127)


def pack(codes):
    """codes [..., D] -> bytes [..., D / 2]: element 2i in the low nibble of byte i"""
    c = codes.to(torch.int32)
    return (c[..., 0::2] | (c[..., 1::2] << 4)).to(torch.uint8)


_DOMAIN = {}


def domain(dtype):
    """{e: the codes T represents at scale byte e}, from dequantize_kv_mxfp4(...).to(dtype).double() == the fp64 value"""
    if dtype not in _DOMAIN:
        codes = torch.arange(32).remainder(16).expand(255, 32)
        e = torch.arange(255)
        got = _F().dequantize_kv_mxfp4(pack(codes), e.to(torch.uint8)[:, None], dtype).double()
        want = value64(codes, e)
        ok = (got == want) & (torch.signbit(got) == torch.signbit(want))
        assert torch.equal(ok[:, :16], ok[:, 16:])
        _DOMAIN[dtype] = {int(x): [c for c in range(16) if ok[x, c]] for x in e}
    return _DOMAIN[dtype]


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_the_domain_is_the_one_written_out(dtype):
    dom = domain(dtype)
    for e in range(255):
        mags = sorted({MAGS[c & 7] for c in dom[e]})
        assert sorted(c ^ 8 for c in dom[e]) == sorted(dom[e]), e               # both signs of each magnitude
        if e in FULL[dtype]:
            assert dom[e] == list(range(16)), e
        else:
            assert tuple(mags) == PARTIAL[dtype].get(e, (0.0,)), (e, mags)


def block_codes(allowed, idx):
    """32 codes: every allowed one (all 16: twice), the rest codes 0 and 8, in an order that differs between blocks"""
    seq = list(allowed) * 2 if len(allowed) == 16 else list(allowed) + [0, 8] * ((32 - len(allowed)) // 2)
    assert len(seq) == 32
    k = (7 * idx) % 32
    seq = seq[k:] + seq[:k]
    return seq[::-1] if idx % 2 else seq


class Step:
    """B sequences of one key: the codes and scale bytes of K and V (CPU), the byte tensors padded to one 32-row tile with
    0xFF (GPU), the one-hot queries, and the cache dequantised to T on the CPU for the 16-bit kernel"""

    def __init__(self, D, dtype, assign, zeros=False):
        nblk = D // 32
        self.B = B = -(-255 // nblk)
        self.D, self.dtype = D, dtype
        dom = domain(dtype)
        self.codes, self.e = [], []
        for which, (mul, off) in enumerate(assign):                            # V, then K
            e = torch.tensor([(idx * mul + off) % 255 for idx in range(B * nblk)])
            assert set(e.tolist()) == set(range(255))
            codes = torch.tensor([block_codes([0, 8] if zeros else dom[int(x)], idx + 3 * which) for idx, x in enumerate(e)])
            self.codes.append(codes.view(B, D))
            self.e.append(e.view(B, nblk))
        self.V64, self.K64 = (value64(c.view(B, nblk, 32), x).view(B, D) for c, x in zip(self.codes, self.e))
        assert torch.isfinite(self.V64).all() and torch.isfinite(self.K64).all()
        tile = lambda t: torch.cat([t.view(B, 1, 1, -1), torch.full((B, 1, 31, t.shape[-1]), FF, dtype=torch.uint8)], dim=2)
        vc, kc = (tile(pack(c)) for c in self.codes)
        vs, ks = (tile(x.to(torch.uint8)) for x in self.e)
        deq = lambda p, s: _F().dequantize_kv_mxfp4(p[:, :, :1], s[:, :, :1], dtype)
        Vt, Kt = deq(vc, vs), deq(kc, ks)
        assert torch.equal(Vt.double().view(B, D), self.V64) and torch.equal(Kt.double().view(B, D), self.K64)   # inside the domain
        poison = lambda t: torch.cat([t, torch.full((B, 1, 31, D), float("nan"), dtype=dtype)], dim=2).cuda()
        self.Kt, self.Vt = poison(Kt), poison(Vt)
        self.pad = [t.cuda() for t in (kc, vc, ks, vs)]
        self.q = torch.eye(D, dtype=dtype, device="cuda").view(1, D, 1, D).expand(B, D, 1, D).contiguous()   # head h asks for element h
        self.sl = torch.ones(B, dtype=torch.int32, device="cuda")

    def reference(self):
        """(O, LSE) of the 16-bit kernel on the dequantised cache"""
        return _M().flash_attention_kvcache(self.q, self.Kt, self.Vt, self.sl, softmax_scale=SCALE, return_lse=True)

    def run(self, call):
        """(O [B, D, 1, D], LSE [B, D, 1]) of the MXFP4 call"""
        B, D = self.B, self.D
        if call == "padded":
            return _F().flash_attention_kvcache_fp4(self.q, *self.pad, self.sl, softmax_scale=SCALE, return_lse=True)
        perm = torch.randperm(B + 2, generator=torch.Generator().manual_seed(B + D))[:B].cuda()
        pools = []
        for t in self.pad:                                                      # a page per sequence, two spare ones of 0xFF
            pool = torch.full((B + 2, *t.shape[1:]), FF, dtype=torch.uint8, device="cuda")
            pool[perm] = t
            pools.append(pool)
        table = perm.to(torch.int32).view(B, 1).contiguous()
        if call == "paged":
            return _F().flash_attention_kvcache_fp4_paged(self.q, *pools, self.sl, table, softmax_scale=SCALE, return_lse=True)
        o, lse = _R().flash_attention_kvcache_fp4_ragged(self.q.view(B, D, D), *pools, rg.cu_of([1] * B, device="cuda"), self.sl,
                                                         table, softmax_scale=SCALE, return_lse=True)
        return o.view(B, D, 1, D), lse.transpose(0, 1).contiguous().view(B, D, 1)


def inexact(st, o):
    """the (scale byte, code) pairs of V that did not come back as their fp64 value"""
    B, D = st.B, st.D
    bad = (o.double().cpu() != st.V64.view(B, 1, 1, D)).any(dim=1).view(B, D)
    e = st.e[0].repeat_interleave(32, dim=1)
    return sorted({(int(x), int(c)) for x, c in zip(e[bad].tolist(), st.codes[0][bad].tolist())})


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("call,D", CALLS, ids=CALL_IDS)
def test_every_scale_byte_element_for_element(call, D, dtype):
    for assign in ASSIGN:
        st = Step(D, dtype, assign)
        assert st.V64.unique().numel() > 150 and (st.V64 == 0).any() and torch.signbit(st.V64[st.V64 == 0]).any()
        for n in (1, 2):
            vck.splits(n)
            o, lse = st.run(call)
            ro, rl = st.reference()
            torch.cuda.synchronize()
            assert torch.equal(o.double().cpu(), st.V64.view(st.B, 1, 1, D).expand(st.B, D, 1, D)), \
                ("O = V: (scale byte, code) not exact", assign, n, inexact(st, o)[:40])
            assert t4.same((o, lse), (ro, rl)), ("the bits of the 16-bit kernel on the dequantised cache", assign, n,
                                                int((lse != rl).sum()), int((o.view(torch.int16) != ro.view(torch.int16)).sum()))
            assert torch.isfinite(lse).all()


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("call,D", CALLS, ids=CALL_IDS)
def test_all_zero_blocks_under_every_scale_byte_give_zeros(call, D, dtype):
    st = Step(D, dtype, ASSIGN[1], zeros=True)
    assert (st.V64 == 0).all() and torch.signbit(st.V64).any()
    for n in (1, 2):
        vck.splits(n)
        o, lse = st.run(call)
        assert (o == 0).all() and torch.isfinite(lse).all() and (lse == 0).all(), n
        assert t4.same((o, lse), st.reference()), n


# ---- the device quantiser at the extremes, and the round trip -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("call", ["padded", "packed"])
def test_device_quantiser_at_the_extremes_and_the_round_trip(call, dtype):
    """test_host_kvcache_fp4.cases as k_new / v_new rows at D = 64, one row per sequence into an empty cache: the bytes the
    append writes, and -- the same call attends over that one key -- O = dequantize_kv_mxfp4 of the appended V row"""
    F = _F()
    D, H = 64, 2
    x = th.cases(dtype)
    assert x.shape[0] % 2 == 0 and torch.isfinite(x.float()).all()
    B = x.shape[0] // 2
    kn, vn = x.view(B, 1, 1, D), x.roll(5, 0).view(B, 1, 1, D).contiguous()
    (kq, kqs), (vq, vqs) = F.quantize_kv_mxfp4(kn), F.quantize_kv_mxfp4(vn)     # on the CPU
    for new, packed_, sc in ((kn, kq, kqs), (vn, vq, vqs)):                        # and the numpy reference's codes
        codes, e = th.np_quantize(new.double().numpy().reshape(B, D))
        assert np.array_equal(th.unpack(packed_.view(B, D // 2)), codes) and np.array_equal(sc.view(B, 2).numpy(), e)
    fi = torch.finfo(dtype)
    assert int(kqs.max()) == int(np.floor(np.log2(fi.max))) - 2 + 127 and int(kqs.min()) == {F16: 101, BF16: 0}[dtype]
    q = torch.zeros(B, H, 1, D, dtype=dtype, device="cuda")
    q[:, 0, 0, 0], q[:, 1, 0, 33] = 1.0, 1.0
    sl = torch.zeros(B, dtype=torch.int32, device="cuda")
    got = [torch.full((B + 3, 1, 32, w), FF, dtype=torch.uint8, device="cuda") for w in (D // 2, D // 2, 2, 2)]
    if call == "padded":
        got = [t[:B].contiguous() for t in got]
        o, lse = F.flash_attention_kvcache_fp4(q, *got, sl, k_new=kn.cuda(), v_new=vn.cuda(), softmax_scale=SCALE, return_lse=True)
        rows = list(range(B))
    else:
        rows = torch.randperm(B + 3, generator=torch.Generator().manual_seed(3))[:B].tolist()
        table = torch.tensor(rows, dtype=torch.int32, device="cuda").view(B, 1)
        o, lse = _R().flash_attention_kvcache_fp4_ragged(q.view(B, H, D), *got, rg.cu_of([1] * B, device="cuda"), sl, table,
                                                         k_new=kn.view(B, 1, D).cuda(), v_new=vn.view(B, 1, D).cuda(),
                                                         softmax_scale=SCALE, return_lse=True)
        o, lse = o.view(B, H, 1, D), lse.transpose(0, 1).contiguous().view(B, H, 1)
    torch.cuda.synchronize()
    want = [torch.full_like(t, FF) for t in got]
    for t, new in zip(want, (kq, vq, kqs, vqs)):
        t[rows, :, 0] = new[:, :, 0].cuda()
    for name, g, w in zip(("k_cache", "v_cache", "k_scale", "v_scale"), got, want):
        assert torch.equal(g, w), (name, int((g != w).sum()))
    # the round trip: one key, so O is the appended V row as the format defines it; the host suite holds that each value is T's
    V64 = value64(torch.from_numpy(th.unpack(vq.view(B, D // 2)).astype(np.int64)).view(B, 2, 32), vqs.view(B, 2)).view(B, D)
    assert torch.equal(F.dequantize_kv_mxfp4(vq, vqs, dtype).double().view(B, D), V64)
    assert torch.isfinite(lse).all()
    bad = (o.double().cpu() != V64.view(B, 1, 1, D)).any(dim=1).view(B, D)
    assert not bad.any(), ("O = the dequantised V row", sorted({(int(a), float(b)) for a, b in zip(
        vqs.view(B, 2).repeat_interleave(32, dim=1)[bad].tolist(), V64[bad].tolist())})[:20])
