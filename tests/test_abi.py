# -*- coding: utf-8 -*-
"""The C-ABI library loads on a machine without a GPU and exports exactly what include/trs.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    txt = open(os.path.join(ROOT, "include", "trs.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(trs_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_functions():
    fns = header_functions()
    assert "trs_score_fwd_bwd" in fns and "trs_topk" in fns and len(fns) >= 15


def test_library_exports_every_declared_symbol():
    from torchrecsys_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in header_functions():
        assert hasattr(lib, name), f"{name} declared in include/trs.h but not exported"


def test_binding_matches_header():
    from torchrecsys_amd import _lib
    assert sorted(_lib.PROTOTYPES) == header_functions()
    lib = _lib.load()
    assert lib.trs_abi_version() == _lib.ABI_VERSION
    assert lib.trs_topk_workspace_bytes(100_000, 10) > 0  # host-only helper: callable without a GPU


def test_struct_layout_matches_header():
    """ctypes mirrors of trs_tables / trs_batch have the C layout (x86-64 SysV: natural alignment)."""
    from torchrecsys_amd import _lib
    assert ctypes.sizeof(_lib.TrsTables) == 4 * 8 + 8 * 8 + 8 * 8 + 2 * 8 + 8 * 8 + 2 * 4
    assert ctypes.sizeof(_lib.TrsBatch) == 5 * 8 + 8 + 4 + 4 + 8
    assert _lib.TrsTables.D.offset == 4 * 8 + 8 * 8 + 8 * 8 + 2 * 8 + 8 * 8
    assert _lib.TrsBatch.err_flag_dev.offset == 56


def test_bad_arguments_return_error_codes_without_a_gpu():
    """Argument validation happens on the host before any launch."""
    from torchrecsys_amd import _lib
    lib = _lib.load()
    T, B = _lib.TrsTables(), _lib.TrsBatch()
    assert lib.trs_score_forward(1, ctypes.byref(T), ctypes.byref(B), None, None, None) == -1
    assert b"NULL" in lib.trs_last_error() or b"table" in lib.trs_last_error()
    assert lib.trs_topk(None, 0, 1, None, None, 0, None) == -1
    assert lib.trs_sample_neg(None, 3, 10, 5, 0, 0, None, None) == -1
    with pytest.raises(_lib.TrsError):
        _lib.check(-1, "x")


def test_tuning_knobs_are_set_through_the_abi_not_the_environment():
    """trs_tuning_set (include/trs.h): every knob of csrc/trs_common.h TrsTuning is settable and resettable by name; an
    unknown name is an error; no source file of the library calls getenv outside the one-time read in api.cpp."""
    from torchrecsys_amd import _lib
    lib = _lib.load()
    src = open(os.path.join(ROOT, "torchrecsys_amd", "csrc", "trs_common.h")).read()
    body = src[src.index("struct TrsTuning {"):src.index("TrsTuning& trs_tuning();")]
    import re
    names = re.findall(r"// TRS_([A-Z0-9_]+) ", body)
    assert len(names) >= 10
    for n in names:
        assert lib.trs_tuning_set(n.encode(), 1, 0) == 0, n
        assert lib.trs_tuning_set(n.encode(), 0, 1) == 0, n
    assert lib.trs_tuning_set(b"NO_SUCH_KNOB", 1, 0) < 0 and b"unknown knob" in lib.trs_last_error()
    with _lib.tuning(GEMM16_TILE=256):
        pass
    csrc = os.path.join(ROOT, "torchrecsys_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h", ".cpp")) and f != "api.cpp":
            assert "getenv(" not in open(os.path.join(csrc, f)).read(), f
    assert open(os.path.join(csrc, "api.cpp")).read().count("getenv(") == 1


def _header_struct_fields(name):
    """Member names of `typedef struct NAME { ... } NAME;` in include/trs.h, in declaration order."""
    import re
    src = open(os.path.join(ROOT, "include", "trs.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        # "float *a, *b"  /  "const void* keys[TRS_MAX_META]"  /  "int32_t x"
        first, *rest = decl.split(",")
        out.append(re.sub(r"\[.*\]", "", first.split()[-1]).lstrip("*"))
        out += [re.sub(r"\[.*\]", "", r_.strip()).lstrip("*").strip() for r_ in rest]
    return out


def test_ctypes_structs_follow_the_header_member_by_member():
    """A ctypes mirror with a member missing or out of order would shift every device pointer after it by one slot."""
    import re
    from torchrecsys_amd import _lib
    for cname, mirror in (("trs_train_args", _lib.TrsTrainArgs), ("trs_opt", _lib.TrsOpt),
                          ("trs_meta_stage", _lib.TrsMetaStage), ("trs_tables", _lib.TrsTables),
                          ("trs_batch", _lib.TrsBatch), ("trs_sampler", _lib.TrsSampler)):
        assert _header_struct_fields(cname) == [f[0] for f in mirror._fields_], cname
    src = open(os.path.join(ROOT, "include", "trs.h")).read()
    assert int(re.search(r"#define TRS_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION
    assert _lib.load().trs_train_steps_sgd(None, None) == -1  # validated on the host, no launch


def _shipped_kernel_registers(tmp_path):
    """{mangled kernel name: (VGPRs, scratch bytes per lane)} of every gfx950 kernel in the shipped library, read from
    its code objects' notes (no GPU, no recompilation)."""
    import re
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("ROCm LLVM tools not found")
    from torchrecsys_amd import _lib
    fat = tmp_path / "fat.bin"
    subprocess.run([tools[0], "-O", "binary", "--only-section=.hip_fatbin", _lib.LIB_PATH, str(fat)], check=True)
    data = fat.read_bytes()
    offs = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), data)]
    assert offs, "no offload bundle in libtrs_hip.so"
    found = {}
    for k, o in enumerate(offs):  # one bundle per translation unit
        part, co = tmp_path / "b.bin", tmp_path / "co.o"
        part.write_bytes(data[o:offs[k + 1] if k + 1 < len(offs) else len(data)])
        r = subprocess.run([tools[1], "--type=o", "--unbundle", f"--input={part}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], capture_output=True)
        if r.returncode:
            continue
        notes = subprocess.run([tools[2], "--notes", str(co)], capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
            sc = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            if name and vg and sc:
                found[name.group(1)] = (int(vg.group(1)), int(sc.group(1)))
    shutil.rmtree(tmp_path, ignore_errors=True)
    return found


def test_one_launch_step_kernels_keep_four_waves_per_simd(tmp_path):
    """Register guard on the shipped code objects (no GPU, no recompilation): the one-launch step kernels of the c4 /
    c2 row shapes (FM, 16-byte lanes, whole rows: 32 or 16 lanes per triple) need at most 128 VGPRs — four waves per
    SIMD; at 133-135 the same kernel ran 2 us per step slower (profiles/EXPERIMENTS.md) — and no scratch."""
    import re
    found = _shipped_kernel_registers(tmp_path)
    hot = {n: v for n, v in found.items()
           if re.search(r"fwd_stage_kernelILi1ELi4ELi(32|16)ELi1ELi0ELb1ELi3ELi0ELi[013]E", n)}
    assert len(hot) == 6, sorted(hot)
    for n, (vgpr, scratch) in hot.items():
        assert vgpr <= 128 and scratch == 0, (n, vgpr, scratch)


def test_retrieval_tile_loop_kernels_keep_their_registers(tmp_path):
    """Register guard for the two kernels that run the shared tile loop of csrc/retrieve.hip: every instance of
    retrieve_topk_kernel<NQ, SELF> and rank_count_kernel<NQ> has no scratch and at most the VGPRs it had when each
    kernel carried its own copy of the loop.  rank_count_kernel<2> sits exactly on the
    128-VGPR line of four waves per SIMD."""
    import re
    found = _shipped_kernel_registers(tmp_path)
    limit = {"retrieve_topk_kernelILi%dELb0E": {2: 188, 4: 195, 8: 211, 16: 245, 32: 256},
             "retrieve_topk_kernelILi%dELb1E": {2: 188, 4: 195, 8: 211, 16: 243, 32: 256},
             "rank_count_kernelILi%dEE": {2: 128, 4: 136, 8: 152, 16: 184, 32: 248}}
    seen = {n: v for n, v in found.items() if re.search(r"\d(retrieve_topk_kernel|rank_count_kernel)I", n)}
    assert len(seen) == 10 + 5, sorted(seen)
    for pat, by_nq in limit.items():
        for nq, most in by_nq.items():
            hit = [n for n in seen if (pat % nq) in n]
            assert len(hit) == 1, (pat % nq, hit)
            vgpr, scratch = seen[hit[0]]
            assert scratch == 0 and vgpr <= most, (hit[0], vgpr, scratch, most)


def test_staged_gradient_kernels_keep_their_waves_per_simd(tmp_path):
    """Register guard for the kernels that stage gradients through the shared pieces of csrc/score_kernels.h (DESIGN.md
    4.1): every instance of score_kernel (MODE 2 lives in fast_step.hip's code object), multineg_kernel and warp_kernel
    in the shipped library has no scratch and at least the waves per SIMD it had when each kernel carried its own copy
    of the slot stager, the loss reduction and the row head.  tests/staged_kernel_waves.json holds those classes per
    instance, read by _shipped_kernel_registers from the library built before the pieces were shared."""
    import json
    import re
    found = _shipped_kernel_registers(tmp_path)
    before = json.load(open(os.path.join(ROOT, "tests", "staged_kernel_waves.json")))
    seen = {n: v for n, v in found.items() if re.search(r"\d(multineg_kernel|warp_kernel|score_kernel)I", n)}
    assert sorted(seen) == sorted(before) and len(seen) == 96 + 48 + 72
    for n, (vgpr, scratch) in seen.items():
        waves = min(8, 512 // (8 * -(-vgpr // 8)))  # 512 VGPRs per lane and SIMD, allocated in blocks of 8
        assert scratch == 0 and waves >= before[n], (n, vgpr, scratch, waves, before[n])


def test_step_kernels_are_the_ones_shipped_before_the_sort_keys_became_32_bit_only(tmp_path):
    """Register guard for the code objects of csrc/fast_step.hip and csrc/presort.hip (no GPU, no recompilation).
    tests/step_kernels.json holds (VGPRs, scratch) of their kernels as built before the sorted references lost their
    key-type template parameter, keyed by the names the kernels have now.  The source of every kernel that is launched
    did not change, so EQUALITY is required: any difference means a kernel was altered by accident.  Gone for good:
    every instance with a 64-bit key type and the stand-alone sorted_user_dup_update_kernel (never launched: the fused
    kernel runs its body) — presort.hip's code object went from 296 kernels to 200."""
    import json
    import re
    found = _shipped_kernel_registers(tmp_path)
    before = json.load(open(os.path.join(ROOT, "tests", "step_kernels.json")))

    def family(n):  # the kernel's own identifier in its mangled name (None: an identifier with digits, none of ours)
        m = re.search(r"(?<=\d)([a-z_]+_kernel)", n)
        return m.group(1) if m else None

    for obj in ("fast_step", "presort"):
        for n, want in before[obj].items():
            assert n in found, (obj, n)
            assert list(found[n]) == want, (obj, n, found[n], want)
    unchanged = {"fwd_stage_kernel", "flagged_update_kernel", "item_owner_update_kernel", "user_plain_update_kernel",
                 "user_dup_update_kernel", "item_update_kernel", "user_update_kernel", "meta_stage_kernel",
                 "pair_scores_kernel", "score_kernel", "sorted_updates_fused_kernel", "cut_rows_apply_kernel",
                 "batch_flags_kernel", "batch_group_items_kernel", "item_flags_kernel", "meta_refs_kernel"}
    lost_key_type = {"epoch_refs_kernel", "sorted_item_update_kernel", "sorted_item_update_staged_kernel",
                     "user_flags_kernel"}
    fams = {obj: {family(n) for n in before[obj]} for obj in before}
    assert fams["fast_step"] | fams["presort"] == unchanged | lost_key_type
    assert fams["presort"] >= lost_key_type
    # no kernel of these families beyond the fixture's (score_kernel also lives in other code objects: presence only)
    for obj in before:
        shipped = {n for n in found if family(n) in fams[obj] - {"score_kernel"}}
        assert shipped == {n for n in before[obj] if family(n) != "score_kernel"}, (obj, sorted(shipped ^ set(before[obj]))[:5])
    assert len(before["presort"]) == 200
    assert not [n for n in found if "sorted_user_dup_update_kernel" in n]
    assert not [n for n in found if family(n) in lost_key_type and re.search(r"_kernelI[jm]", n)]  # no key-type argument
