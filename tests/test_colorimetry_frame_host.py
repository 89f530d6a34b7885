"""The format word of vt_frame.format (csrc/vt_frame.hpp: validation and splitting in one place - family, layout, name, row
bytes, chroma helpers, level, and the colour code's place in the layout word) in a stand-alone program of its own,
tests/colorimetry_frame_main.cpp, compiled with AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process.
No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gstreamer-vit-tracker_amd", "csrc")


def test_format_word_helpers_under_sanitizers(tmp_path):
    exe = tmp_path / "colorimetry_frame_main"
    # the runtimes linked statically: the program then starts whatever else the environment preloads into processes
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe),
                    os.path.join(ROOT, "tests", "colorimetry_frame_main.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith(", 0 checks failed"), r.stdout[-4000:] + r.stderr[-4000:]
