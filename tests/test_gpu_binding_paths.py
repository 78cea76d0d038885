"""Every branch of the decode bindings' shared call path (csrc/torch_binding_decode.h: prepare_inputs, prepare_launch), once per
binding module and geometry, at the smallest shape that still crosses a page and ends in a partial tile: B 2, H 4, H_kv 2,
D 64, pages of 32 keys, cache lengths 33 and 40, S_q 1 for the padded and paged calls and packed rows (1, 3) for the packed ones.

q contiguous, strided but addressable in place (a head-transposed view) and misaligned by one element (the binding copies it);
k_new / v_new absent and non-contiguous (the binding copies them); a packed call's `out` absent and strided, written in place.
Every result has the bits of the same call on contiguous clones, the appended cache rows and scales agree bit for bit, and the
contiguous call is within the modules' own fp64 bound (fp8tokencheck.BOUND with test_gpu_kvcache.check_lse, quantcapcheck.check
for the capped calls).  The caches, calls and truths are quantcapcheck's: its Cache covers the three quantised formats, its
plain_* adapters reach _mi355fa_fp4_torch, _mi355fa_fp8_token_torch and (per-tensor e4m3 pools) _mi355fa_paged_torch, its capped
ones _mi355fa_quant_softcap_torch."""
import pytest
import torch

import fp8tokencheck as tk
import quantcapcheck as qc
import raggedcheck as rg

pytestmark = pytest.mark.gpu

B, H, HKV, D, PAGE, LENS, ROWS, CAP = 2, 4, 2, 64, 32, [33, 40], [1, 3], 30.0
# (binding module, cache format, geometries): the per-tensor e4m3 padded call is torch_binding.cpp's, not a decode binding's
MODULES = [("fp4", "fp4", ("padded", "paged", "packed")), ("fp8_token", "token", ("padded", "paged", "packed")),
           ("paged", "e4m3", ("paged", "packed")), ("quant_softcap", "e4m3", ("padded", "paged", "packed")),
           ("quant_softcap", "token", ("padded", "paged", "packed")), ("quant_softcap", "fp4", ("padded", "paged", "packed"))]
CASES = [(m, f, g) for m, f, geoms in MODULES for g in geoms]


def _call(mod, geom, q, c, sl, table, cu, **kw):
    if mod == "quant_softcap":
        if geom == "packed":
            return qc.Q().flash_attention_kvcache_quant_softcap_ragged(q, c.k, c.v, cu, sl, table, CAP, return_lse=True, **c.kw(), **kw)
        return qc.padded(q, c, sl, CAP, **kw) if geom == "padded" else qc.paged(q, c, sl, table, CAP, **kw)
    if geom == "packed":
        return qc.plain_packed(q, c, cu, sl, table, **kw)
    return qc.plain_padded(q, c, sl, **kw) if geom == "padded" else qc.plain_paged(q, c, sl, table, **kw)


def _layouts(t):
    """t contiguous -> (a strided view the kernels address in place, a view one element off the 16-byte boundary), same values"""
    swapped = t.transpose(0, 1).contiguous().transpose(0, 1)        # heads outermost in memory
    off = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape)
    off.copy_(t)
    assert not swapped.is_contiguous() and swapped.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 2 and off.is_contiguous()
    return swapped, off


def _wide(t):
    """t -> the same values as a non-contiguous view (rows twice as far apart)"""
    w = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)[..., :t.shape[-1]]
    w.copy_(t)
    assert not w.is_contiguous()
    return w


def _same_cache(a, b):
    return all(torch.equal(qc.bits(x), qc.bits(y)) for x, y in zip(a.tensors(), b.tensors()))


@pytest.mark.parametrize("dtype", tk.DT, ids=tk.IDS)
@pytest.mark.parametrize("mod,fmt,geom", CASES, ids=["%s-%s-%s" % c for c in CASES])
def test_every_layout_gives_the_bits_of_the_contiguous_call(mod, fmt, geom, dtype):
    packed, capped = geom == "packed", mod == "quant_softcap"
    Sq = max(ROWS) if packed else 1
    q4, cache = qc.make(fmt, B, H, HKV, Sq, 2 * PAGE, D, dtype, CAP, seed=11)
    sl, table, cu, c = qc.sl_of(LENS), None, None, cache
    if geom != "padded":
        c, table = qc.scatter(cache, LENS, PAGE, 2, seed=3, alloc=[2 * PAGE] * B)
    if packed:
        qs = [q4[b:b + 1, :, :s].contiguous() for b, s in enumerate(ROWS)]
        q, cu = rg.pack(qs, sum(ROWS)), rg.cu_of(ROWS, device="cuda")
    else:
        qs, q = None, q4.contiguous()
    ref = _call(mod, geom, q, c.clone(), sl, table, cu)

    # the contiguous call against fp64 on the dequantised cache
    per_seq = list(zip(rg.unpack(ref[0], ROWS), rg.unpack_lse(ref[1], ROWS))) if packed else [ref]
    for b, (o, lse) in enumerate(per_seq):
        qb, cb, lens = (qs[b], cache.rows(b, LENS[b]), [LENS[b]]) if packed else (q, cache, LENS)
        if capped:
            qc.check("%s %s %s" % (mod, fmt, geom), qb, o, lse, qc.truth(qb, cb, lens, CAP), lens, matters=False)
        else:
            K, V = cb.deq64()
            tk.held("%s %s" % (mod, geom), qb, o, lse, *tk.truth(qb, K, V, lens), lens)

    # q addressed in place through its strides, and q copied
    for layout in _layouts(q):
        assert tk.same(_call(mod, geom, layout, c.clone(), sl, table, cu), ref)

    # k_new / v_new non-contiguous, q strided: the bits, and the appended rows and scales, of the call on contiguous clones
    kn, vn = qc.new_rows(B, HKV, Sq, D, dtype, seed=7)
    if packed:
        kn, vn = (rg.pack([t[b:b + 1, :, :s] for b, s in enumerate(ROWS)], sum(ROWS)) for t in (kn, vn))
    ca, cb = c.clone(), c.clone()
    want = _call(mod, geom, q, ca, sl, table, cu, k_new=kn.contiguous(), v_new=vn.contiguous())
    got = _call(mod, geom, _layouts(q)[0], cb, sl, table, cu, k_new=_wide(kn), v_new=_wide(vn))
    assert tk.same(got, want)
    assert _same_cache(ca, cb) and not _same_cache(ca, c)      # the same rows and scales, and the append did write

    # a packed call's `out`: strided, written in place
    if packed:
        out = _wide(torch.zeros_like(q))
        o, lse = _call(mod, geom, q, c.clone(), sl, table, cu, out=out)
        assert o.data_ptr() == out.data_ptr() and o.stride() == out.stride()
        assert tk.same((out.contiguous(), lse), ref)
