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


def test_kept_copies_are_still_there():
    """KEPT lists only what is really kept: an entry whose copy has gone is removed from the list."""
    src = _sources()
    for name, kept in KEPT.items():
        for needle in kept:
            assert needle in _code(src[name]), (name, needle)
