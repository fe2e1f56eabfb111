"""the CPU-side C under AddressSanitizer + UndefinedBehaviorSanitizer.

  * oracle/msnap_oracle.c (the checker every parity test leans on) is rebuilt with
    -fsanitize=address,undefined and the oracle-golden tests are re-run against that build in a python
    started with libasan preloaded: an out-of-bounds access or undefined arithmetic in the restatement
    would otherwise pass silently into every "parity" number.
  * the HOST side of the C-ABI (csrc/msnap_api.hip compiled for the host only, kernel launchers replaced
    by stand-ins that abort if reached) is built the same way and driven through every entry point's
    argument checks and the create/destroy error paths by a plain-C program (tests/c_abi/abi_args.c).
GPU AddressSanitizer is not available on the pool: device code is covered by the parity tests only."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

ORACLE = os.path.join(ROOT, "oracle")
CSRC = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


def _libasan():
    gcc = shutil.which("gcc")
    if not gcc:
        return None
    p = subprocess.run([gcc, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


def test_c_oracle_under_address_and_ub_sanitizers():
    asan = _libasan()
    if asan is None or not shutil.which("make"):
        pytest.skip("no gcc / libasan here")
    subprocess.run(["make", "-C", ORACLE, "sanitize"], check=True, capture_output=True)
    lib = os.path.join(ORACLE, "libmsnap_oracle_san.so")
    # libasan first (the runtime must be the first library loaded), whatever the environment preloads kept behind it
    preload = ":".join(p for p in (asan, os.environ.get("LD_PRELOAD")) if p)
    env = dict(os.environ, LD_PRELOAD=preload, MSNAP_ORACLE_LIB=lib, OMP_NUM_THREADS="4",
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    # the C oracle against the reference-generated goldens, the order-9 extended-precision fixture and the
    # full-size formation fixtures (sampler + both collision passes), all through the sanitized library
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "not gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_oracle_golden.py"),
                        os.path.join(ROOT, "tests", "test_formation_full.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "passed" in r.stdout and "ERROR: AddressSanitizer" not in tail and "runtime error" not in tail, tail
    # and the sanitized library is really the one that was loaded
    probe = ("import sys; sys.path.insert(0, %r); import c_oracle; c_oracle.load(); "
             "print(open('/proc/self/maps').read().count('libmsnap_oracle_san.so') > 0)" % ORACLE)
    r = subprocess.run([sys.executable, "-c", probe], env=env, capture_output=True, text=True)
    assert r.stdout.strip().endswith("True"), r.stdout + r.stderr


def test_c_abi_host_side_incl_limits_under_address_and_ub_sanitizers(tmp_path):
    """Every C-ABI entry point, the dynamic-limits ones included (csrc/msnap_api.hip hosts them all; the stand-ins
    of tests/c_abi/host_stubs.cpp follow the launcher declarations of csrc/msnap_internal.h)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    exe = str(tmp_path / "abi_args_san")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", CSRC]
    objs = []
    for src, extra in [(os.path.join(CSRC, "msnap_api.hip"), ["-x", "hip", "--offload-host-only", "-std=c++17"]),
                       (os.path.join(ROOT, "tests", "c_abi", "host_stubs.cpp"), ["-x", "hip", "--offload-host-only", "-std=c++17"]),
                       (os.path.join(ROOT, "tests", "c_abi", "abi_args.c"), ["-x", "c"])]:
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([hipcc, *extra, *SAN, *inc, "-c", src, "-o", obj], check=True, capture_output=True)
        objs.append(obj)
    subprocess.run([hipcc, *SAN, *objs, "-o", exe], check=True, capture_output=True)
    # every device hidden: on a machine with a GPU msnap_create would otherwise get as far as the kernel-setup stand-in
    # of host_stubs.cpp, which aborts; hidden, the program takes the no-device path it is written for everywhere
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               LSAN_OPTIONS="suppressions=" + os.path.join(ROOT, "tests", "c_abi", "lsan.supp"),
               HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "abi_args: 0 failure(s)" in r.stdout, out[-3000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
