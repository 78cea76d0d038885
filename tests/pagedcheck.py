"""Helpers of the paged-KV-cache tests (tests/test_host_paged.py, tests/test_gpu_paged.py, tests/test_gpu_paged_deep.py;
not a test module): a padded cache [B, H_kv, S, D] scattered into a pool of pages [num_pages, H_kv, page, D] through a
random table, and gathered back.  The pool is built so that a stray read shows as a NaN, never as a fault: every page no
sequence uses and every row past a sequence's length in its last page is NaN, every table entry past a sequence's pages
points at a NaN page, and scatter() never draws an out-of-range entry.  wide_table() is the same table as a slice of a
wider one (a row stride above max_pages, a base off 16 bytes); guarded() is the same pool as the middle of a larger
NaN-filled allocation, so that a test which plants entries a few pages outside [0, num_pages) on purpose would see a
missing range check as a NaN or a changed guard byte, not as a fault.  Works on any device and for 16-bit and
float8_e4m3fn caches (whose NaN is the byte 0x7f)."""
import torch


def _bytes(t):
    """`t` as integers of its element size: indexing and comparing without NaN semantics"""
    return t.view({1: torch.uint8, 2: torch.int16}[t.element_size()])


def fill_nan(t):
    """every element of `t` (a 16-bit or e4m3 tensor, or a view of one) = NaN, in place"""
    if t.element_size() == 1:
        _bytes(t).fill_(0x7f)
    else:
        t.fill_(float("nan"))
    return t


def pages_of(L, page):
    return -(-L // page)


def scatter(caches, lens, page, num_pages, max_pages, seed, table=None, alloc=None):
    """caches: padded [B, H_kv, S, D] tensors (K and V) sharing one table; lens[b]: the rows of sequence b that count
    (<= S and <= max_pages * page).  Returns (pools, table): pools [num_pages, H_kv, page, D] like each cache and the int32
    table [B, max_pages] on the caches' device.  Sequences get distinct random pages for ceil(lens[b] / page) entries; the
    rest of each row names a page no sequence uses (there is at least one).  table given: use that table (e.g. rows that
    share pages) instead of drawing one; every page it does not name within a sequence's entries stays NaN.  alloc[b] >=
    lens[b]: the keys sequence b gets pages for (room for an append: the rows past lens[b] are NaN all the same)."""
    B, Hkv, S, D = caches[0].shape
    dev = caches[0].device
    used = [pages_of(L, page) for L in (alloc or lens)]
    assert all(L <= S and n <= max_pages and n * page >= L for L, n in zip(lens, used))
    if table is None:
        assert sum(used) < num_pages, "keep at least one page unused"
        g = torch.Generator().manual_seed(seed)
        perm = torch.randperm(num_pages, generator=g).tolist()
        spare = perm[sum(used):]
        table = torch.empty(B, max_pages, dtype=torch.int32)
        at = 0
        for b in range(B):
            for i in range(max_pages):
                table[b, i] = perm[at + i] if i < used[b] else spare[(b + i) % len(spare)]
            at += used[b]
    pools = []
    for c in caches:
        pool = fill_nan(torch.empty(num_pages, Hkv, page, D, dtype=c.dtype, device=dev))
        for b in range(B):
            for i in range(pages_of(lens[b], page)):
                n = min(page, lens[b] - i * page)
                _bytes(pool)[int(table[b, i]), :, :n] = _bytes(c)[b, :, i * page:i * page + n]
        pools.append(pool)
    return pools, table.to(dev)


def gather(pool, table, lens=None):
    """The padded cache [B, H_kv, max_pages * page, D] a pool and a table describe (bytes copied, so NaN pages stay as they
    are).  lens given: rows at or past lens[b] are zeroed."""
    num_pages, Hkv, page, D = pool.shape
    B, max_pages = table.shape
    out = _bytes(pool)[table.long()]                                   # [B, max_pages, H_kv, page, D]
    out = out.permute(0, 2, 1, 3, 4).reshape(B, Hkv, max_pages * page, D).contiguous()
    if lens is not None:
        for b, L in enumerate(lens):
            out[b, :, L:] = 0
    return out.view(pool.dtype)


def unused_pages(table, lens, page, num_pages):
    """the pages no sequence names within its first ceil(lens[b] / page) entries, ascending (scatter left them NaN)"""
    t = table.cpu()
    used = {int(t[b, i]) for b, L in enumerate(lens) for i in range(pages_of(L, page))}
    return [n for n in range(num_pages) if n not in used]


def wide_table(table, fill, left=3, right=4):
    """`table` [B, max_pages] as the columns [left, left + max_pages) of a new int32 [B, left + max_pages + right] tensor
    on its device whose other columns name the pages of `fill` in turn (in-range NaN pages: a lookup that ignores the row
    stride or the base shows as a NaN).  The view has the same entries, stride(0) > size(1), and with left = 3 a base 12
    bytes past the allocation's: 4-byte aligned, not 16."""
    B, mp = table.shape
    fill = torch.tensor(list(fill), dtype=torch.int32)
    wide = fill[torch.arange(B * (left + mp + right)) % len(fill)].view(B, left + mp + right).to(table.device)
    wide[:, left:left + mp] = table
    return wide[:, left:left + mp]


def guarded(pool, guard):
    """(big, view): `pool`'s bytes as pages [guard, guard + num_pages) of a new allocation of num_pages + 2 * guard pages
    whose other pages are NaN, and the view of those pages (contiguous, the same shape and dtype as `pool`)"""
    n = pool.shape[0]
    big = fill_nan(torch.empty(n + 2 * guard, *pool.shape[1:], dtype=pool.dtype, device=pool.device))
    _bytes(big)[guard:guard + n] = _bytes(pool)
    return big, big[guard:guard + n]


def guards_intact(big, guard):
    """every byte of the 2 * guard pages around a guarded() pool is still the NaN fill"""
    fresh = fill_nan(torch.empty_like(big[:guard]))
    return same_bytes(big[:guard], fresh) and same_bytes(big[big.shape[0] - guard:], fresh)


def move_pages(pool, perm):
    """a new pool with page n of `pool` at perm[n] (perm: an int64 permutation of the pages on the pool's device)"""
    return torch.empty_like(_bytes(pool)).index_copy_(0, perm, _bytes(pool)).view(pool.dtype)


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bytes(a), _bytes(b))
