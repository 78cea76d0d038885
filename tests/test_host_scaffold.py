"""The kernels' shared scaffolding is written once (DESIGN.md "Scaffolding: written once"): plain string search over the
csrc sources that holds the fold in place.  A copy that stays on purpose -- hipcc compiled the shared form to other
instructions in a kernel of the strict-identity tier -- is listed in KEPT with its reason; nothing else may come back."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd", "csrc")

# file -> {what stays: why}
_PERSISTENT = ("its own Work / decode / tile-order lambdas (the persistent work list): decoded through a shared struct or "
               "function the kernel compiled to other instructions in the release or a diagnostic build")
KEPT = {
    "fa_fwd_v4.hip": {"xcd_remap(": _PERSISTENT},
    "fa_bwd_dq_v4.hip": {"xcd_remap(": _PERSISTENT},
    "fa_bwd_dkv_v4.hip": {"xcd_remap(": _PERSISTENT},
}


def _sources():
    files = sorted(p for ext in ("*.hip", "*.inc", "*.h") for p in glob.glob(os.path.join(CSRC, ext)))
    assert len(files) >= 20
    return {os.path.basename(p): open(p).read() for p in files}


def _code(text):
    """The text without // comments (the sources have no block comments that matter here)."""
    return re.sub(r"//.*", "", text)


def _files_with(needle, code_only=True):
    return sorted(n for n, t in _sources().items() if needle in (_code(t) if code_only else t))


def test_multiprocessor_count_is_queried_in_one_file():
    assert _files_with("hipDeviceAttributeMultiprocessorCount") == ["fa_kernels.h"]
    users = _files_with("persistent_grid(")
    assert users == ["fa_bwd_dkv_v2.hip", "fa_bwd_dkv_v4.hip", "fa_bwd_dq_v4.hip", "fa_fwd_v4.hip", "fa_kernels.h"], users


def test_lds_opt_in_mask_lives_in_the_launch_helper():
    assert _files_with("opted_in") == ["fa_kernels.h"]
    # every kernel with a dynamic LDS carve is launched through the helper
    for name, text in _sources().items():
        if name != "fa_kernels.h" and "hipFuncSetAttribute" in _code(text):
            raise AssertionError(name)


def test_cycle_counter_is_read_in_the_stamps_header_only():
    assert _files_with("s_memtime", code_only=False) == ["fa_stamps.h"]
    assert _files_with("s_memrealtime", code_only=False) == ["fa_stamps.h"]


def test_one_stamp_macro_body():
    bodies = []
    for name, text in _sources().items():
        flat = text.replace("\\\n", " ")
        for m in re.finditer(r"#\s*define\s+(\w*STAMP\w*)\(slot\)(.*)", flat):
            if "seg[slot]" in m.group(2):
                bodies.append((name, m.group(1)))
    assert bodies == [("fa_stamps.h", "FA_STAMP")], bodies
    # and no kernel file defines a stamp macro of its own
    for name, text in _sources().items():
        if name != "fa_stamps.h":
            assert not re.search(r"#\s*define\s+\w*STAMP", text), name


def test_work_list_is_decoded_in_the_helpers_only():
    callers = [n for n in _files_with("xcd_remap(") if n != "fa_kernels.h"]
    assert callers == sorted(n for n, kept in KEPT.items() if "xcd_remap(" in kept), callers
    # the kernels that walk a work list go through the helpers
    users = set(_files_with("tile_index<CAUSAL>(")) | set(_files_with("tile_index_item<CAUSAL>("))
    assert users >= {"fa_fwd_body.inc", "fa_bwd_dq_body.inc", "fa_bwd_dkv_body.inc", "fa_fwd_v2.hip", "fa_fwd_v3.hip",
                     "fa_bwd_dq_v3.hip", "fa_bwd_dkv_v2.hip", "fa_bwd_dkv_v3.hip"}, users


def test_fence_lambdas_are_gone():
    for name, text in _sources().items():
        code = _code(text)
        assert not re.search(r"auto\s+(tile_sync|pipe_sync)\s*=", code), name
    assert "FA_DEVINL void tile_sync()" in _sources()["fa_common.h"]
    assert "FA_DEVINL void pipe_sync()" in _sources()["fa_common.h"]


def test_no_wait_is_a_bare_number():
    """Every s_waitcnt immediate goes through waitcnt_imm(), every counted vmcnt is an expression of named request counts."""
    for name, text in _sources().items():
        assert "s_waitcnt(0x" not in text, name
        code = _code(text)
        assert not re.search(r"__builtin_amdgcn_s_waitcnt\(\s*0[xX]", code), name
        for m in re.finditer(r"vmcnt\((\d+)", code):   # an asm string: vmcnt(0) or vmcnt(%0) with an "n" operand
            assert m.group(1) == "0", (name, m.group(0))


def test_epilogue_store_counts_share_the_store_loop_bound():
    src = _sources()
    body = re.search(r"FA_DEVINL void store_tile_rows\(.*?\n}\n", src["fa_common.h"], re.S).group(0)
    assert "i < kTileRowStores<D>;" in _code(body)
    for name in ("fa_bwd_dq_v4.hip", "fa_bwd_dkv_v4.hip"):
        assert re.search(r"kEpilogueStores = \d \* kTileRowStores<D>;", _code(src[name])), name


def test_ring_rotation_is_written_once():
    assert _files_with("b2 = bt") == ["fa_common.h"]
    assert _files_with("ring_rotate(b0, b1, b2)") == ["fa_bwd_dkv_v4.hip", "fa_bwd_dq_v4.hip"]


def test_wait_ledger_names_what_the_kernels_wait_for():
    """DESIGN.md's ledger: every row's expression stands in the kernel it names, and every counted wait of the three
    family-4 kernels -- a waitcnt_imm() of something other than 0 / kNoWait, an asm vmcnt(%0) -- has a row."""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    table = [line for line in design.split("#### The wait ledger\n", 1)[1].split("\n## ", 1)[0].splitlines() if line.startswith("|")]
    rows = [[c.strip() for c in line.strip("|").split("|")] for line in table[2:]]
    assert rows and all(len(r) == 5 for r in rows), rows
    src = _sources()
    for kernel in ("fa_fwd_v4.hip", "fa_bwd_dq_v4.hip", "fa_bwd_dkv_v4.hip"):
        code = _code(src[kernel])
        mine = [r for r in rows if r[0] == "`%s`" % kernel]
        for r in mine:
            quoted = re.findall(r"`([^`]+)`", r[4])
            assert quoted and all(q in code for q in quoted), r
        waited = set(re.findall(r"waitcnt_imm\((?!0\b|kNoWait\b)([^,)]+)", code)) | set(re.findall(r'vmcnt\(%0\)" ::"n"\(([^)]+)\)', code))
        assert waited, kernel
        for w in waited:
            assert any(w.split("::")[-1] in r[4] for r in mine), (kernel, w)


def test_decode_host_path_is_written_once():
    """DESIGN.md "The decode path: written once", the second fold: the MXFP4 launch path is the shared one."""
    everything = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(CSRC, "*"))
                  if p.endswith((".hip", ".inc", ".h", ".cpp")) or os.path.basename(p) == "Makefile"}
    for name, text in everything.items():
        assert "launch_decode_fp4" not in text, name
    decode = _code(_sources()["fa_decode.hip"])
    assert len(re.findall(r"hipLaunchKernelGGL\(\(fa_decode_combine_kernel<", decode)) == 1
    assert decode.count("fa_decode_combine_kernel<") == 1
    assert len(re.findall(r"hipLaunchKernelGGL\(\(fa_decode_combine_ragged_kernel<", decode)) == 1
    assert decode.count("fa_decode_combine_ragged_kernel<") == 1
    # kvcache_impl takes what a call has beside its tensors as one struct: no defaulted parameter
    decl = re.search(r"static int kvcache_impl\((.*?)\)\s*{", _code(_sources()["fa_api.hip"]), re.S).group(1)
    assert "=" not in decl and "const KvCall&" in decl, decl
    # and the bindings raise through one definition
    defs = sorted(n for n, t in everything.items() if re.search(r"\bvoid assertion\(", _code(t)))
    assert defs == ["torch_binding_common.h"], defs
    assert sorted(n for n, t in everything.items() if re.search(r"#\s*define\s+FA_ASSERT\b", t)) == ["torch_binding_common.h"]


def test_kept_copies_are_still_there():
    """KEPT lists only what is really kept: an entry whose copy has gone is removed from the list."""
    src = _sources()
    for name, kept in KEPT.items():
        for needle in kept:
            assert needle in _code(src[name]), (name, needle)
