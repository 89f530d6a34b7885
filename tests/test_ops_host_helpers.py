"""The host arithmetic of the operator hooks (csrc/vt_ops_host.hpp: bf16 rounding, the 3-byte pair, the timing hooks'
operand generators, the cfg split) in a stand-alone program of its own, tests/ops_host_main.cpp, compiled with
AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process. No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gstreamer-vit-tracker_amd", "csrc")


def test_the_host_header_is_pure_cxx17():
    """no HIP, nothing of the engine: what lets the program below be built by g++ alone"""
    txt = open(os.path.join(CSRC, "vt_ops_host.hpp")).read()
    includes = [l.split()[1] for l in txt.splitlines() if l.startswith("#include")]
    assert includes and all(i.startswith("<") for i in includes), includes
    assert "hip" not in " ".join(includes)


def test_host_helpers_under_sanitizers(tmp_path):
    exe = tmp_path / "ops_host_main"
    # the runtimes linked statically: the program then starts whatever else the environment preloads into processes
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe),
                    os.path.join(ROOT, "tests", "ops_host_main.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 checks failed"), r.stdout[-4000:] + r.stderr[-4000:]
