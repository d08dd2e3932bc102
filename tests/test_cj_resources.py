"""What the flagship closure-join variant (k_closure_join<24, 2048, 32, true>, the kernel behind
bench.py's figure) takes of a CU: no scratch, and no more than the 80 VGPRs and 24,096 B of LDS
that let 6 of its blocks (24 waves) share a CU. (The 64-VGPR / 20,480-B variant with 8 blocks per
CU was built and measured no faster, DESIGN §3.1, so the bound is the 6-block one.) Read from the
metadata notes of libgck_kernels.co with llvm-readelf, as tests/test_aql_codeobject.py reads the
kernarg layout. No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CO = os.path.join(ROOT, "gochugaru_amd", "libgck_kernels.co")
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
FLAGSHIP = "void gck::k_closure_join<24, 2048u, 32u, true>(gck::Ctx, gck::CjArgs)"


def _flagship():
    if not os.path.exists(CO):
        pytest.skip("libgck_kernels.co not built")
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf missing")
    cf = shutil.which("c++filt")
    if not cf:
        pytest.skip("c++filt missing")
    notes = subprocess.run([READELF, "--notes", CO], capture_output=True, text=True, check=True).stdout
    blocks = {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in notes.split("  - .agpr_count:")[1:]}
    names = list(blocks)
    dm = subprocess.run([cf], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_dm = dict(zip(dm, names))
    assert FLAGSHIP in by_dm, "the flagship variant is not in the code object"
    block = blocks[by_dm[FLAGSHIP]]
    # (.agpr_count opens each kernel's record: it is the text the split consumed)
    out = {"agpr_count": int(re.match(r"\s*(\d+)", block).group(1))}
    for k in ("vgpr_count", "vgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size"):
        out[k] = int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
    return out


def test_flagship_join_fits_six_blocks_per_cu():
    r = _flagship()
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    assert r["vgpr_count"] <= 80 and r["agpr_count"] == 0, r  # 512 registers per lane and SIMD: 6 waves
    assert r["group_segment_fixed_size"] <= 24096, r    # 160 KB per CU: 6 blocks
