"""The key table of the peak arbitration (csrc/vt_feature_keys.hpp: kArbKeys and apply_arbitrate - bounds, defaults,
refusal texts, unknown keys, untouched words on a refusal) in a stand-alone program of its own, tests/arbitrate_keys_main.cpp,
compiled with AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process. No GPU, nothing loaded into
Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gstreamer-vit-tracker_amd", "csrc")


def test_arbitrate_key_table_under_sanitizers(tmp_path):
    exe = tmp_path / "arbitrate_keys_main"
    # the runtimes linked statically: the program then starts whatever else the environment preloads into processes
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe),
                    os.path.join(ROOT, "tests", "arbitrate_keys_main.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 checks failed"), r.stdout[-4000:] + r.stderr[-4000:]
