"""tools/isa_lint.py: the counted-wait LDS kernels (gemm3.hip / gemm4_<type>.hip) compiled for gfx950 must
have no VGPR hazard on an in-flight inline-asm LDS read and no -Winline-asm warning (the VERDICT r4
gemm4 root cause: dead next-stage reads of a split's last stage had their registers recycled while
the LDS data was still in flight).  CPU only: hipcc cross-compiles the device assembly."""
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_lint as L  # noqa: E402

SNIPPET_BAD = """
_Zkernel:
\t;;#ASMSTART
\tds_read_b128 v[4:7], v1
\t;;#ASMEND
\t;;#ASMSTART
\tds_read_b128 v[8:11], v1 offset:16
\t;;#ASMEND
\ts_waitcnt lgkmcnt(1)
\tv_mfma_f32_32x32x16_f16 v[16:31], v[4:7], v[0:3], v[16:31]
\tv_add_u32_e32 v9, 4, v2
\ts_cbranch_scc0 .LBB0_2
\ts_waitcnt lgkmcnt(0)
.LBB0_2:
\tv_mov_b32_e32 v40, v8
\ts_endpgm
.Lfunc_end0:
"""

SNIPPET_OK = """
_Zkernel:
\t;;#ASMSTART
\tds_read_b128 v[4:7], v1
\t;;#ASMEND
\ts_load_dword s4, s[0:1], 0x10
\t;;#ASMSTART
\tds_read_b128 v[8:11], v1 offset:16
\t;;#ASMEND
\t;;#ASMSTART
\tds_read_b128 v[8:11], v1 offset:32
\t;;#ASMEND
\ts_waitcnt lgkmcnt(2)
\tv_mfma_f32_32x32x16_f16 v[16:31], v[4:7], v[0:3], v[16:31]
\ts_waitcnt lgkmcnt(0)
\tv_mov_b32_e32 v40, v8
\ts_endpgm
.Lfunc_end0:
"""


def _lint_text(tmp_path, text):
    p = tmp_path / "k.s"
    p.write_text(text)
    k = L.parse(str(p))
    insns, labels = k["_Zkernel"]
    return L.analyse(insns, labels)


def test_lint_flags_clobber_and_stale_read(tmp_path):
    findings, infos, overflow = _lint_text(tmp_path, SNIPPET_BAD)
    kinds = sorted(k for (_, k) in findings)
    # v9 written while v[8:11] is in flight; v8 read on the branch path that skipped the wait
    assert kinds == ["clobber", "read"], findings
    assert not overflow


def test_lint_accepts_counted_waits(tmp_path):
    findings, infos, overflow = _lint_text(tmp_path, SNIPPET_OK)
    assert findings == {}
    assert len(infos) == 1   # lgkmcnt(2) with the s_load in flight: reported, not a finding
    assert not overflow


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None,
                    reason="hipcc not available")
def test_gemm_kernels_isa_clean(tmp_path):
    """Compile gemm3.hip and the per-type gemm4 units to gfx950 assembly (in parallel, ~3 min) and
    lint every kernel instantiation: zero findings, zero -Winline-asm warnings."""
    srcs = L.default_sources()
    assert len(srcs) == 7, srcs   # gemm3 + the six weight types of gemm4
    with ThreadPoolExecutor(4) as ex:
        outs = list(ex.map(lambda s: L.compile_asm(s, str(tmp_path)), srcs))
    assert sum(w for _, w in outs) == 0, "-Winline-asm warnings"
    total = 0
    for path, _ in outs:
        with open(path) as f:
            assert re.search(r"gemm[34]_kernel", f.read()), path + ": no kernel to lint"
        total += L.lint_file(path, r"gemm[34]_kernel", verbose=False)
    assert total == 0
