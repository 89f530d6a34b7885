"""The key tables of the keyed optional features (csrc/vt_feature_keys.hpp: bounds, defaults, refusal texts, the derived
thresholds, the packed overlay style, the frozen thumbnail size, the operator hooks' check_words) in a stand-alone program of its own,
tests/feature_keys_main.cpp, compiled with AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process.
No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gstreamer-vit-tracker_amd", "csrc")


def test_the_key_header_is_pure_cxx17():
    """no HIP, nothing of the engine: what lets the program below be built by g++ alone"""
    txt = open(os.path.join(CSRC, "vt_feature_keys.hpp")).read()
    includes = [l.split()[1] for l in txt.splitlines() if l.startswith("#include")]
    assert includes and all(i.startswith("<") for i in includes), includes
    assert "hip" not in " ".join(includes)


def test_key_tables_under_sanitizers(tmp_path):
    exe = tmp_path / "feature_keys_main"
    # the runtimes linked statically: the program then starts whatever else the environment preloads into processes
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe),
                    os.path.join(ROOT, "tests", "feature_keys_main.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 checks failed"), r.stdout[-4000:] + r.stderr[-4000:]
