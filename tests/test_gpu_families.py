"""The fixed-length schedule families 1, 2 and 3 against fp64, block by block, at the shapes the automatic rule sends them to.

The generated table (csrc/fa_table.h) and the fallbacks of fa_kernels.h pick_*_impl choose families 1-3 for most cells of
the (B * H, S) grid.  Every case below runs under the automatic rule (nothing forced), and fa_debug_pick / fa_debug_pick_ex
must answer the family the case names for each kernel.  test_every_family_the_rule_produces_has_a_case walks every cell
of the rule (square, ragged, S_q != S_k both ways) on the CPU and fails if the rule produces a (kernel, D, dtype, causal,
family) no case runs -- a new table from tools/tune.py --emit needs a case before it lands.  The case list also has every
causal family with tile pairing on and off (want_pairs restated with the launcher's own tile), every launch of a family
1-3 kernel has more workgroups than the MI355X has CUs, and each kernel runs at least one case at S >= 8192.

The checks are those of test_gpu_blockwise.py (blockcheck.py): the raw C entry points with every output NaN-filled, twice
(bit-identical), bf16 once more with the q_scaled workspace, and the autograd function once (its O / dQ the bits of the raw
launch, its dK / dV those of the launch with the workspace); every (batch, head, 128-row block) of O, dQ, dK and dV
against fa_oracle.attention_fp64_chunked on the device, LSE per row within a + u * SABS, delta per row against
rowsum(dO * O) of the kernel's own O; rows that are exactly 0 in fp64 (V = 0 heads, dO = 0 heads, keys no query sees)
exactly 0.

Per-block relative Frobenius errors measured on an MI355X over every case here, as largest block / largest per-case
median block ("raw" = without the workspace, "ws" = with it, which the autograd path equals bit for bit):

                  fp16 D = 64      fp16 D = 128     bf16 D = 64      bf16 D = 128
    O             4.5e-4/2.9e-4    3.4e-4/2.9e-4    5.5e-3/2.9e-3    5.1e-3/2.9e-3
    dQ            9.2e-4/3.1e-4    5.5e-4/3.1e-4    6.2e-3/3.0e-3    5.5e-3/2.9e-3
    dK  raw       8.3e-4/3.2e-4    7.8e-4/3.1e-4    1.6e-2/3.2e-3    1.4e-2/3.0e-3
    dK  ws                                          1.2e-2/3.4e-3    6.1e-3/3.3e-3
    dV  raw       5.5e-4/2.9e-4    3.7e-4/3.0e-4    1.7e-2/3.0e-3    2.0e-2/2.9e-3
    dV  ws                                          9.9e-3/2.9e-3    6.1e-3/2.9e-3

The largest block is at most 3.7x the median of its group.  Rows that see fewer than 8 keys (checked row by row, see
test_gpu_blockwise.py) reach 1.5e-2 (fp16, the family-4 dQ of dkv-causal-fp16) and 4.0e-2 (bf16); LSE is within 0.3 of
its bound a + u * SABS on every row, delta within 1.8e-7 relative of rowsum(dO * O).  On one MI355X the GPU tests of this
file take about 6 s.  The bounds below sit about 1.5x above the largest errors."""
import itertools

import pytest
import torch

import fa_oracle as fo
from blockcheck import (BF16, DKV, DQ, F16, FWD, KERNEL_NAMES, _lib, assert_family, check_outputs, few_rows, grid_size,
                        launch_plain, launch_plain_autograd, make_inputs, same_bits, want_pairs)

# (B, H, S_q, S_k, D, dtype, causal, families (fwd, dQ, dK/dV) under the automatic rule, id)
CASES = [
    # the short-sequence cells at B * H = 200 and 512 (S = 180: one full and one 52-row tile)
    (8, 25, 180, 180, 64, F16, False, (1, 3, 2), "bh200-s180-fp16-d64"),
    (8, 25, 180, 180, 64, BF16, False, (1, 3, 2), "bh200-s180-bf16-d64"),
    (8, 25, 180, 180, 128, F16, False, (1, 1, 2), "bh200-s180-fp16-d128"),
    (8, 25, 180, 180, 128, BF16, False, (1, 1, 2), "bh200-s180-bf16-d128"),
    (8, 25, 180, 180, 64, F16, True, (3, 1, 2), "bh200-s180-causal-fp16-d64"),
    (8, 25, 180, 180, 128, F16, True, (1, 1, 1), "bh200-s180-causal-fp16-d128"),
    (8, 25, 180, 180, 128, BF16, True, (1, 1, 1), "bh200-s180-causal-bf16-d128"),
    (8, 25, 180, 250, 128, F16, True, (1, 1, 2), "bh200-sq<sk-causal-fp16-d128"),
    (8, 25, 180, 250, 128, BF16, True, (1, 1, 2), "bh200-sq<sk-causal-bf16-d128"),
    (16, 32, 180, 53, 64, F16, False, (1, 3, 1), "bh512-sq>sk-fp16-d64"),
    (16, 32, 180, 53, 128, F16, False, (1, 1, 1), "bh512-sq>sk-fp16-d128"),
    (16, 32, 180, 53, 128, BF16, False, (1, 1, 1), "bh512-sq>sk-bf16-d128"),
    (16, 32, 180, 53, 64, F16, True, (3, 1, 1), "bh512-sq>sk-causal-fp16-d64"),
    (16, 32, 180, 53, 64, BF16, True, (3, 1, 1), "bh512-sq>sk-causal-bf16-d64"),
    (16, 32, 180, 250, 64, F16, False, (2, 1, 2), "bh512-sq<sk-fp16-d64"),
    (16, 32, 180, 250, 64, BF16, False, (1, 1, 1), "bh512-sq<sk-bf16-d64"),
    (16, 32, 180, 250, 64, BF16, True, (1, 3, 2), "bh512-sq<sk-causal-bf16-d64"),
    # mid-length cells, ragged on both sides
    (8, 16, 700, 831, 64, BF16, False, (2, 3, 3), "bh128-s700-bf16-d64"),
    (3, 16, 700, 831, 64, BF16, False, (3, 3, 2), "bh48-s700-bf16-d64"),
    (8, 25, 700, 831, 64, BF16, True, (1, 3, 3), "bh200-s700-causal-bf16-d64"),
    (4, 15, 631, 531, 64, F16, True, (1, 3, 2), "bh60-sq>sk-causal-fp16-d64"),
    (3, 16, 1500, 1423, 64, F16, False, (4, 3, 3), "bh48-s1500-fp16-d64"),
    (2, 6, 2800, 2723, 64, F16, False, (3, 3, 2), "bh12-s2800-fp16-d64"),
    (2, 16, 2800, 2931, 64, F16, True, (1, 3, 3), "bh32-s2800-causal-fp16-d64"),
    (8, 32, 1100, 1100, 64, F16, False, (2, 3, 2), "bh256-s1100-fp16-d64"),
    (16, 32, 1000, 1151, 64, BF16, False, (1, 3, 3), "bh512-s1000-bf16-d64"),
    (16, 32, 2053, 2053, 64, F16, True, (1, 3, 2), "bh512-s2053-causal-fp16-d64"),
    # fallback edges at large grids
    (4, 32, 4096, 4001, 64, BF16, False, (4, 3, 3), "dq-ragged-keys-bf16"),             # dQ 4 -> 3: S_k % 128 != 0
    (4, 32, 4096, 4000, 64, BF16, True, (1, 3, 3), "fwd-uncovered-tile-causal-bf16"),  # fwd 4 -> 1, dQ 4 -> 3, dK/dV 4 -> 3
    (4, 32, 4096, 4096, 64, F16, True, (1, 4, 3), "dkv-causal-fp16"),                  # the fp16 causal dK/dV: family 3
    (4, 32, 3000, 4096, 64, BF16, True, (4, 4, 3), "dkv-causal-sq<sk-bf16"),           # dK/dV 4 -> 3: S_q < S_k
    # S >= 8192
    (2, 16, 8197, 8131, 64, F16, True, (1, 3, 3), "s8197-causal-fp16-d64"),
    (2, 16, 8192, 8061, 128, BF16, True, (1, 1, 2), "s8192-causal-bf16-d128"),
    (1, 32, 9001, 8192, 128, F16, False, (4, 1, 2), "s9001-fp16-d128"),
]

# Per-block error bounds by (dtype, output), about 1.5x the largest block measured over CASES (module docstring).
BLOCK_BOUND = {
    (F16, "O"): 7e-4, (F16, "dQ"): 1.4e-3, (F16, "dK"): 1.25e-3, (F16, "dV"): 8.5e-4,
    (BF16, "O"): 8.5e-3, (BF16, "dQ"): 9.5e-3, (BF16, "dK"): 1.8e-2, (BF16, "dV"): 1.5e-2,
}
BOUNDS = dict(BLOCK_BOUND=BLOCK_BOUND, BLOCK_BOUND_RAW_BF16_DKV=3e-2, FEW_BOUND={F16: 2.3e-2, BF16: 6e-2}, RATIO=4.0,
              FLOOR=1e-5, LSE_BOUND={F16: (1e-4, 0.0), BF16: (1e-3, 2.0 ** -8)}, DELTA_BOUND=1e-6)


def cu_count():
    """The MI355X's CUs: every family 1-3 launch of a case must have more workgroups."""
    return 256


def run_case(case, check=True, seed=0):
    B, H, Sq, Sk, D, dtype, causal, fams, tag = case
    _, lib = _lib()
    for k in (FWD, DQ, DKV):
        assert lib.fa_debug_pick(k, D, int(dtype == BF16), int(causal), B, H, Sq, Sk) == fams[k], (tag, KERNEL_NAMES[k])
        assert_family(k, fams[k], D, dtype, causal, B, H, Sq, Sk)
    Q, K, V, dO, groups = make_inputs(B, H, H, Sq, Sk, D, dtype, seed)
    gt = fo.attention_fp64_chunked(Q, K, V, dO, causal)
    few = few_rows(fo.visible_mask(Sq, Sk, (-1, 0) if causal else (-1, -1), "cuda"))
    cw = dict(check=check, V=V, few=few)
    run = lambda got, mode: check_outputs("%s %s" % (tag, mode), gt, got, dO, groups, groups, dtype, mode, BOUNDS, **cw)
    raw = launch_plain(Q, K, V, dO, causal, workspace=False)
    raw2 = launch_plain(Q, K, V, dO, causal, workspace=False)
    for n in ("O", "LSE", "delta", "dQ", "dK", "dV"):
        assert same_bits(raw[n], raw2[n]), (tag, n, "second launch")
    recs = run(raw, "raw")
    ref = raw
    if dtype == BF16:
        ws = launch_plain(Q, K, V, dO, causal, workspace=True)
        assert not torch.isnan(ws["qs"]).any(), (tag, "the dQ launch left q_scaled rows unwritten")
        for n in ("O", "LSE", "delta", "dQ"):
            assert same_bits(raw[n], ws[n]), (tag, n, "the workspace changes only dK / dV")
        recs += run(ws, "ws")
        ref = ws
    ag = launch_plain_autograd(Q, K, V, dO, causal)
    recs += run(ag, "autograd")
    for n in ("O", "dQ", "dK", "dV"):
        assert same_bits(ag[n], ref[n]), (tag, n, "autograd and the raw launch")
    for r in recs:
        r.update(dtype="bf16" if dtype == BF16 else "fp16", D=D, causal=causal, fams=fams)
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize("case", [pytest.param(c, id=c[-1]) for c in CASES])
def test_families_1_to_3_blocks_against_fp64(case):
    run_case(case)


# ---------------------------------------------------------------- the case list against the rule (CPU)
def rule_combinations():
    """Every (kernel, D, dtype, causal, family in 1-3) the automatic rule produces over the (B * H, S) buckets of
    fa_table.h: each cell square, with ragged tails off the 128 / 256 multiples, and with S_q != S_k both ways."""
    _, lib = _lib()
    out = set()
    for (B, H), S in itertools.product(((1, 8), (2, 16), (4, 32), (16, 32)), (128, 256, 512, 1024, 2048, 4096, 8192, 16384)):
        for Sq, Sk in ((S, S), (S - 3, S - 3), (S + 5, S + 5), (S, S - 77), (S - 77, S), (S - 3, S), (S, S - 3)):
            for k, D, dt, c in itertools.product((FWD, DQ, DKV), (64, 128), (0, 1), (0, 1)):
                f = lib.fa_debug_pick(k, D, dt, c, B, H, Sq, Sk)
                if f in (1, 2, 3):
                    out.add((k, D, dt, c, f))
    return out


def test_every_family_the_rule_produces_has_a_case():
    _, lib = _lib()
    lib.fa_debug_force_impl(0, 0, 0)
    have = set()
    for B, H, Sq, Sk, D, dtype, causal, fams, tag in CASES:
        for k in (FWD, DQ, DKV):
            assert lib.fa_debug_pick(k, D, int(dtype == BF16), int(causal), B, H, Sq, Sk) == fams[k], (tag, KERNEL_NAMES[k])
            have.add((k, D, int(dtype == BF16), int(causal), fams[k]))
    missing = sorted(rule_combinations() - have)
    assert not missing, "no case in tests/test_gpu_families.py runs (kernel, D, dtype, causal, family): %s" % missing


def test_case_list_reaches_pairs_large_grids_and_long_sequences():
    """Every causal family runs paired and unpaired (where the launcher has a choice), every family 1-3 launch has more
    workgroups than CUs, every kernel runs at S >= 8192, and the fallback edges the module docstring lists are there."""
    seen, long_s = set(), set()
    for B, H, Sq, Sk, D, dtype, causal, fams, tag in CASES:
        for k in (FWD, DQ, DKV):
            f = fams[k]
            if max(Sq, Sk) >= 8192:
                long_s.add(k)
            if f == 4:
                continue
            assert grid_size(k, f, B, H, Sq, Sk, causal) > cu_count(), (tag, KERNEL_NAMES[k])
            if causal:
                seen.add((k, f, want_pairs(k, f, B, H, Sq, Sk, causal)))
    for k, f, _, _, _ in {(k, f, 0, 0, 0) for k, f, _ in seen}:
        always = k != DKV and f == 2
        assert (k, f, True) in seen and (always or (k, f, False) in seen), (KERNEL_NAMES[k], f)
    assert long_s == {FWD, DQ, DKV}
    by_id = {c[-1]: c for c in CASES}
    assert by_id["dq-ragged-keys-bf16"][7][DQ] == 3 and by_id["fwd-uncovered-tile-causal-bf16"][7][FWD] == 1
    assert by_id["dkv-causal-fp16"][7][DKV] == 3 and by_id["dkv-causal-sq<sk-bf16"][7][DKV] == 3
