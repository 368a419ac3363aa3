"""What the host-emulation tests share (test infrastructure): kernels compiled for the HOST against tests/hip_host_shim (one thread
per lane, pthread barriers) into a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer, run as a child
process.  The compiler is the one that builds the library."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "hip_host_shim")
CSRC = os.path.join(ROOT, "eabnet_amd", "csrc")


def _compiler():
    for c in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"), shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    raise AssertionError("no clang++ (the compiler of the ROCm installation that builds the library)")


def build(tmp_path_factory, name: str, *sources: str) -> str:
    """the program ``name``_emulation of shim.cpp + ``name``_main.cpp and the csrc files ``sources`` compiled as C++; without
    sources the main includes its kernels itself and finds them in csrc"""
    exe = str(tmp_path_factory.mktemp(f"{name}_emulation") / f"{name}_emulation")
    kernels = ["-x", "c++", *(os.path.join(CSRC, s) for s in sources)] if sources else ["-I", CSRC]
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", SHIM, "-I", os.path.join(ROOT, "include"), *kernels,
           os.path.join(SHIM, "shim.cpp"), os.path.join(SHIM, f"{name}_main.cpp"), "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run(program: str, *args: str, timeout: int = 600) -> None:
    """one child process; a sanitizer report or a refused call is a non-zero exit status"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([program, *args], capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
