"""CPU: the C-ABI library builds for gfx950, loads without a GPU, exports exactly the symbols
include/sehip.h declares, and the product path refuses to run without a device (no fallback)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "sehip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(se_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    import sehip
    lib = sehip.lib()
    declared = header_symbols()
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(sehip.EXPORTS) == declared
    assert lib.se_version() >= 100
    assert lib.se_build_arch() == b"gfx950"


def test_code_object_targets_gfx950():
    import sehip
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", sehip.LIB_PATH], capture_output=True, text=True)
    strings = subprocess.run(["strings", sehip.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in strings or "gfx950" in out.stdout


def test_no_cpu_fallback():
    import torch
    import sehip
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    x = torch.randn(4, 8)
    with pytest.raises(sehip.SehipError):
        sehip.normalize_rows_(x)
    with pytest.raises(sehip.SehipError):
        sehip.cosine_embedding_loss(x, torch.zeros(4, dtype=torch.long), torch.randn(3, 8))
    import evaluate_retrieval
    with pytest.raises(sehip.SehipError):
        evaluate_retrieval.pairwise_retrieval(np.random.rand(5, 3).astype(np.float32), return_generator=False)


def test_argument_validation_without_gpu():
    """Host-side checks of the C ABI run before any launch: exercise them with null pointers."""
    import ctypes
    import sehip
    lib = sehip.lib()
    z = ctypes.c_void_p(0)
    assert lib.se_pairwise_dist(z, 4, z, 4, z, z, 2, 2, 4, 0, None, 0, z, 2, z) == -1
    assert b"null pointer" in lib.se_last_error()
    assert lib.se_topk_rows(z, 4, 1, 4, 0, 9999, z, z, z) == -1
    assert lib.se_rank_rows_workspace_bytes(50000, 50000) > 0
    assert lib.se_rank_rows(z, 0, 0, 0, z, 0, 0, z, 0, z) == 0     # empty problem is OK
    kb = (ctypes.c_int32 * 2)(3, 4)
    one = ctypes.c_void_p(16)
    assert lib.se_pairwise_dist(one, 8, one, 8, z, z, 2, 2, 8, 0, kb, 2, one, 2, z) == -1   # blocks sum to 7 != 8
    assert b"K-blocks" in lib.se_last_error()
    # the l2norm backward decides the epsilon clamp from the forward's sum x^2, which it cannot do without
    assert lib.se_l2norm_bwd(one, 8, one, 8, one, z, 2, 8, one, 8, z) == -1
    assert b"se_l2norm_bwd" in lib.se_last_error()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "semantic-embeddings_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(dirpath, f)


def test_product_library_carries_no_tuning_switches():
    """The product .so ignores every tuning / ablation environment variable (none of their names is even compiled in); the
    -DSE_TUNING build next to it -- loaded only by tests / tools through SEHIP_LIB -- honours them.  SE_RANK_SAFE / SE_RANK_VERBOSE
    are product switches (guaranteed-order ranking kernel, probe verdict)."""
    import sehip
    from sehip import _lib
    product = subprocess.run(["strings", os.path.join(os.path.dirname(_lib.TUNING_LIB_PATH), "libsehip.so")], capture_output=True, text=True).stdout
    tuning = subprocess.run(["strings", _lib.TUNING_LIB_PATH], capture_output=True, text=True).stdout
    for name in ("SE_PD_ABLATE", "SE_PD_NOSTAGGER", "SE_PD_PLAIN_ST", "SE_PD_PROFILE", "SE_RR_PROFILE", "SE_RANK_PEEL", "SE_RANK_TILED",
                 "SE_TOPK_EXACT"):
        assert name not in product, name
        assert name in tuning, name
    assert "SE_RANK_SAFE" in product
    assert "pdist_ws" not in product          # the slower wave-specialised experiment is not shipped
    assert not os.path.exists(os.path.join(ROOT, "semantic-embeddings_amd", "csrc", "pdist_ws.hip"))


def test_tuning_library_exports_the_same_abi():
    import ctypes
    from sehip import _lib
    lib = ctypes.CDLL(_lib.TUNING_LIB_PATH)
    for name in header_symbols():
        assert hasattr(lib, name), name


def test_no_unsynchronised_function_local_state_in_the_library():
    """include/sehip.h promises re-entrancy: function-local statics of the host code are const (thread-safe one-time
    initialisation) or atomics."""
    csrc = os.path.join(ROOT, "semantic-embeddings_amd", "csrc")
    bad = []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h")):
            continue
        for ln, line in enumerate(open(os.path.join(csrc, f)), 1):
            m = re.match(r"\s+static\s+(?!const\b|constexpr\b|thread_local\b|std::atomic|__device__|inline\b)(\w[\w:<> \*]*)\s+\w+.*[=;]", line)
            if m and "std::mutex" not in line and "guarded by mu" not in line and "(" not in line.split("=")[0]:
                bad.append("%s:%d: %s" % (f, ln, line.strip()))
    assert not bad, bad


def test_every_work_group_barrier_drains_the_lds_queue_first():
    """Round 4 bug: one barrier of the LDS bitonic sort was compiled without `s_waitcnt lgkmcnt(0)` on its loop back edge and
    se_topk_rows returned unsorted rows under two-stream contention.  Every kernel now goes through wg_barrier() (se_common.h);
    the audit reads the SHIPPED code objects, and the sources may not go back to a bare barrier."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_barrier_audit
    import sehip
    kernels, barriers, bare = isa_barrier_audit.audit(sehip.LIB_PATH)
    assert barriers > 500 and len(kernels) > 100, (barriers, len(kernels))        # the audit did see the kernels
    assert not bare, bare[:5]
    assert isa_barrier_audit.hazards(sehip.LIB_PATH) == []                         # the path-sensitive form of the same question
    csrc = os.path.join(ROOT, "semantic-embeddings_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith(".hip"):
            src = re.sub(r"//.*", "", open(os.path.join(csrc, name)).read())
            assert not re.search(r"__syncthreads\s*\(\s*\)|__builtin_amdgcn_s_barrier", src), name


def test_ranking_kernels_fit_the_instruction_cache():
    """Round 6: the 98-key instantiations of the register-resident ranking kernel were 66.8 / 68.6 KB of code against a 64 KB
    instruction cache; whether the per-row loop thrashed it depended on where the code object placed the kernel (identical code:
    7.2 or 8.0 ms, profiles/r06_b_rank_icache.txt).  The hardware-ordered instantiations the benchmark shapes take (up to 98 keys
    per thread, every variant) must stay below the cache's 64 KB in the SHIPPED library (total code: the per-row loop is smaller -- the
    canonical-key fallback, the outlier list, the int64 / uint16 write-outs and the long-run repair are cold; the round's last
    addition, 64.0 / 65.0 KB in all, still measures ~1.7 k SQC_ICACHE_MISSES per dispatch)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_barrier_audit
    import sehip
    sizes = isa_barrier_audit.kernel_code_bytes(sehip.LIB_PATH)
    rank = {k: v for k, v in sizes.items() if "rank_rows_reg_kernel" in k}
    assert len(rank) >= 40, len(rank)
    seen = 0
    for name, size in rank.items():
        m = re.search(r"rank_rows_reg_kernelILi(\d+)ELb0ELb1ELi(\d)ELb0", name)      # <ITEMS, PROF = false, HWORD = true, VAR, SEG = false>
        if m and int(m.group(1)) <= 98:
            seen += 1
            assert size < 64 * 1024, (name, size)
    assert seen >= 30, seen

