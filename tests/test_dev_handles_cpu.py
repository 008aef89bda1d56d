"""CPU: the resource handles of csrc/h2g_dev.h (device memory, page-locked memory, events, streams) driven over malloc / free under the host sanitizers
(tests/dev/dev_check.cpp, which defines the eight HIP entry points the handles call: no HIP runtime is linked, no GPU is needed); the unit that uses them keeps no
hand-written release of its own."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hisat2_amd", "csrc")


def _rocm_path():
    """ROCM_PATH, or the tree the Makefile's HIPCC lives in"""
    if os.environ.get("ROCM_PATH"):
        return os.environ["ROCM_PATH"]
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
    return os.path.dirname(os.path.dirname(hipcc))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dev") / "dev_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(_rocm_path(), "include"), "-o", exe, os.path.join(ROOT, "tests", "dev", "dev_check.cpp")], check=True)
    return exe


def test_handles_under_sanitizers(checker):
    """ensure / reserve / reset (the free comes before the allocation; a failed allocation leaves an empty buffer that the next call fills), moves and release, and a context
    of mixed handles built with its k-th creation failing, for every k: nothing stays live, nothing is freed twice, every stream goes after every buffer and event; no leak at
    exit (ASan)"""
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]


def test_the_header_stands_alone():
    """h2g_dev.h includes the HIP runtime's API header and nothing of the project"""
    inc = re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', open(os.path.join(CSRC, "h2g_dev.h")).read(), re.M)
    assert "hip/hip_runtime_api.h" in inc and not [i for i in inc if i.startswith("h2g")]


def test_partitioned_areas_under_sanitizers(checker):
    """csrc/h2g_parts.h in the same program: reset / fits / lo / hi of an area in parts, a failed allocation that leaves no area, and the spans the cursors describe
    (nothing touched, a cursor at its part's start, a part in the middle, a cursor beyond its part, the last part), every expected number written out by hand"""
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    assert int(re.search(r"the areas in parts, (\d+) checks", r.stdout).group(1)) >= 20


def test_the_parts_header_stands_alone():
    """h2g_parts.h includes h2g_dev.h and nothing else of the project"""
    inc = re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', open(os.path.join(CSRC, "h2g_parts.h")).read(), re.M)
    assert [i for i in inc if i.startswith("h2g")] == ["h2g_dev.h"] and not [i for i in inc if "/" in i]


def test_the_c_abi_unit_releases_nothing_by_hand():
    """every device buffer, event and stream of h2g_kernels.hip is a handle: the unit itself names no release call (h2g_host_free hands raw page-locked memory back to a caller)"""
    src = open(os.path.join(CSRC, "h2g_kernels.hip")).read()
    for call in ("hipFree(", "hipEventDestroy(", "hipStreamDestroy(", "hipMalloc("):
        assert call not in src, call
    assert src.count("hipHostFree(") == 1 and src.count("hipHostMalloc(") == 1
