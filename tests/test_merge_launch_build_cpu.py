"""What the built library's code object says about how pk_rank_merge_nostore is launched: no private segment (a wave that asks for
scratch waits for its allocation at launch, and the kernel never touches any), at most 64 vector registers (8 waves per SIMD) and no
vector spills.  Reads the kernels' metadata notes, never an instruction:
the gfx950 code object is cut out of the library's offload bundle here and handed to llvm-readelf --notes."""
import os
import re
import shutil
import struct
import subprocess

import pytest

from phylo_amd import _ffi

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "max_flat_workgroup_size",
          "uses_dynamic_stack")


def readelf():
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"), os.path.join("/opt/rocm", "llvm", "bin")):
        p = os.path.join(d, "llvm-readelf")
        if os.path.exists(p):
            return p
    return shutil.which("llvm-readelf")


def code_object(blob):
    """The gfx950 entry of the (uncompressed) offload bundle inside the library"""
    at = blob.find(MAGIC)
    assert at >= 0, "no offload bundle in the library"
    n, = struct.unpack_from("<Q", blob, at + len(MAGIC))
    p = at + len(MAGIC) + 8
    for _ in range(n):
        off, size, tlen = struct.unpack_from("<QQQ", blob, p)
        p += 24
        triple = blob[p:p + tlen].decode()
        p += tlen
        if "gfx950" in triple:
            return blob[at + off:at + off + size]
    raise AssertionError("no gfx950 code object in the bundle")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(_ffi.LIB_PATH):
        pytest.skip("%s is not built" % _ffi.LIB_PATH)
    tool = readelf()
    assert tool, "llvm-readelf (ROCm's LLVM) not found"
    with open(_ffi.LIB_PATH, "rb") as f:
        co = code_object(f.read())
    path = tmp_path_factory.mktemp("co") / "gfx950.elf"
    path.write_bytes(co)
    text = subprocess.run([tool, "--notes", str(path)], check=True, capture_output=True, text=True).stdout
    out = {}
    # one YAML map per kernel inside amdhsa.kernels: a list item opens with "  - ", its keys are sorted
    for block in re.split(r"\n\s+- \.", text):
        m = re.search(r"\.name:\s+(\S+)", block)
        if not m:
            continue
        d = {}
        for key in FIELDS:
            v = re.search(r"\b%s:\s+(\S+)" % key, block)
            if v:
                d[key] = v.group(1)
        out[m.group(1)] = d
    return out


def merge_kernels(kernels):
    """every pk_rank_merge_nostore the library ships (one today: a wave per workgroup), not the id-resolving pk_rank_merge_nostore_ids"""
    return {name: d for name, d in kernels.items() if re.match(r"_Z21pk_rank_merge_nostore(P|I)", name)}


def test_one_wave_per_workgroup(kernels):
    ks = merge_kernels(kernels)
    assert len(ks) == 1
    for name, d in ks.items():
        assert int(d["max_flat_workgroup_size"]) == 64, (name, d)


def test_no_private_segment_eight_waves_no_vector_spills(kernels):
    ks = merge_kernels(kernels)
    assert ks
    for name, d in ks.items():
        assert int(d["private_segment_fixed_size"]) == 0, (name, d)
        assert d["uses_dynamic_stack"] == "false", (name, d)
        assert int(d["vgpr_count"]) <= 64, (name, d)
        assert int(d["vgpr_spill_count"]) == 0, (name, d)


def test_the_neighbours_stay_without_one(kernels):
    """the chain bookkeeping of the flagship and its scan read 0 bytes before this kernel did"""
    seen = 0
    for name, d in kernels.items():
        if name.startswith("_Z24pk_rank_book_chain_cladeILi8EE") or name.startswith("_Z20pp_resample_scan_ancILi512EE"):
            assert int(d["private_segment_fixed_size"]) == 0, (name, d)
            seen += 1
    assert seen == 2
