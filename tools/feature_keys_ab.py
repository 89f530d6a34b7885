"""The keyed optional features (result overlay, motion prior, appearance check, reacquire proposals) and response peaks
on two builds of libvittrack_hip.so, call for call: the return code, the vt_last_error text and every value read back
must be the same. One child process per library; tiny model, 2 tracked streams (and a third that is never initialised),
640 x 480 synthetic NV12.
usage: python tools/feature_keys_ab.py --build-parent [REV [DIR]]  (anywhere, in a git checkout) -> REV's (default HEAD~1)
                                                              sources exported to DIR (default build/parent, git-ignored)
                                                              and built there; prints the library's path
       python tools/feature_keys_ab.py LIB_A LIB_B            (on the GPU box) -> the report, "0 differences" at its end
       python tools/feature_keys_ab.py --objects LIB_A LIB_B  (anywhere) -> the gfx950 code objects of both libraries as
                                                              SHA-256 multisets, and both vt_build_info strings
LIB_A is usually the parent commit's library from --build-parent, LIB_B this tree's. For --objects both libraries must have been built at the same path, one after the
other: hipcc derives each translation unit's id, which its code object carries, from the path of the source."""
import collections
import hashlib
import json
import os
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, W, H = 2, 640, 480
FEATURES = {
    # on key, (key, lowest, highest) of every field, an unknown key under the prefix, the stats tensor and its length
    "result overlay": ("result_overlay", [("result_overlay", 0, 7), ("result_overlay_luma", 0, 255), ("result_overlay_rgb", 0, 0xFFFFFF),
                                          ("result_overlay_min_score_pct", 0, 100), ("result_overlay_style", 1 | 1 << 8 | 1 << 16, 16 | 64 << 8 | 4 << 16)],
                       "result_overlay_colour", "result_overlay", 6),
    "motion prior": ("motion_prior", [("motion_prior", 0, 1), ("motion_gain_pct", 1, 100), ("motion_coast", 0, 60), ("motion_max_pct", 0, 200)],
                     "motion_blur", "motion", 8),
    "appearance check": ("appearance", [("appearance", 0, 1), ("appearance_period", 1, 1000000), ("appearance_gate_pm", 0, 1000)],
                         "appearance_gate", "appearance", 8),
    "reacquire proposals": ("proposals", [("proposals", 0, 2), ("proposals_period", 1, 1000000), ("proposals_max", 1, 8),
                                          ("proposals_min_sim_pm", 0, 1000), ("proposals_max_cells", 16384, 4194304)],
                            "proposals_min_sim", "proposals", 60),
}


def child():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import gstreamer_vit_tracker_amd as vt
    lib = vt.lib()
    scs = [vt.synth.MovingSquare(W, H, 64, seed=s) for s in range(B)]
    g = vt.Group(vt.weights.ensure_weights("tiny"), n_streams=B + 1)     # stream B stays uninitialised
    keep = []

    def frames(t):
        keep[:] = [torch.from_numpy(sc.frame_nv12(t)).cuda() for sc in scs]
        return [vt.frame_nv12(d.data_ptr(), d.data_ptr() + W * H, W, H) for d in keep]

    for s, f in enumerate(frames(0)):
        g.init_device(s, f, vt.BBox.new(*scs[s].gt_box(0)))

    def say(what, rc, values=None):
        print(json.dumps([what, int(rc), lib.vt_last_error().decode(), values]), flush=True)

    def tune(key, value):
        say(f"set_tuning {key} {value}", lib.vt_group_set_tuning(g._h, key.encode(), int(value)))

    def read(name, stream, cap):
        """cap None: null out"""
        out = np.full(max(cap or 1, 1), -12345.0, np.float32)
        rc = lib.vt_group_read_tensor(g._h, stream, name.encode(), vt._f32(out) if cap is not None else None, cap or 0)
        say(f"read_tensor {name} stream {stream} cap {cap}", rc, [repr(float(v)) for v in out])

    def peaks(n=B):
        out = np.zeros(n, vt.PEAKS_DTYPE)
        say(f"last_peaks {n}", lib.vt_group_last_peaks(g._h, out.ctypes.data, n), out.tobytes().hex())

    clock = [0]

    def a_pass():
        clock[0] += 1
        res = g.update_device(frames(clock[0]), streams=list(range(B)))
        say(f"pass {clock[0]}", 0, [[repr(float(v)) for v in (*r.bbox, r.score)] for r in res])

    def keys(rows, unknown):
        for key, lo, hi in rows:
            for value in (-1, lo, hi, lo - 1, hi + 1, -1):
                tune(key, value)
        tune(unknown, 1)

    for name, (on, rows, unknown, tensor, n) in FEATURES.items():
        say(f"---- {name}", 0)
        off_first = [r for r in rows if r[0] != on]
        keys(off_first, unknown)            # not capable: kept on the host
        for value in (-1, 0, rows[0][2] + 1):
            tune(on, value)
        read(tensor, 0, None)
        read(tensor, 0, n)
        if name == "reacquire proposals":
            tune("proposals_max_cells", 65536)
        tune(on, rows[0][2])                # the enable, with the highest legal value
        say("graph_captures", g.graph_captures())
        read(tensor, 0, None)
        read(tensor, 1, n - 1)
        read(tensor, 1, n)
        a_pass()
        read(tensor, 0, n)
        keys(rows, unknown)                 # capable: every accepted value is one small copy
        read(tensor, 1, n)
        tune(on, rows[0][2])
        if name == "reacquire proposals":
            for value in (-1, 16384, 65536, 4194305):
                tune("proposals_max_cells", value)
            read(tensor, 0, n)
        if name == "appearance check":
            for value in (-2, B + 1, B, 0, -1):
                tune("appearance_anchor", value)
            read("anchor", 0, None)
            read(tensor, 0, n)
        if name == "motion prior":
            for _ in range(3):
                a_pass()
            read(tensor, 0, n)
            tune(on, 0)
            read(tensor, 0, n)
            read(tensor, 1, n)
            tune(on, 1)
    say("---- response peaks", 0)
    peaks()
    say("set_peaks 0 before the enable", lib.vt_group_set_peaks(g._h, -1, 0, 2, 0.0))
    say("set_peaks radius 9", lib.vt_group_set_peaks(g._h, -1, 3, 9, 0.0))
    peaks()
    say("set_peaks 3", lib.vt_group_set_peaks(g._h, -1, 3, 2, 0.0))
    say("graph_captures", g.graph_captures())
    peaks()
    a_pass()
    peaks()
    say("set_peaks 0 on stream 1", lib.vt_group_set_peaks(g._h, 1, 0, 2, 0.0))
    a_pass()
    peaks()
    peaks(1)
    for tensor, n in (("result_overlay", 6), ("motion", 8), ("appearance", 8), ("proposals", 60)):
        read(tensor, 0, n)
        read(tensor, 1, n)
    g.close()


def run_child(lib):
    env = dict(os.environ, VITTRACK_HIP_LIB=os.path.abspath(lib))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:       # nothing more is started on the GPU behind a child that failed
        print(f"the child on {lib} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        sys.exit(3)
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("[")]


def behaviour(lib_a, lib_b):
    ra, rb = run_child(lib_a), run_child(lib_b)
    print(f"A: {lib_a}\nB: {lib_b}\n{len(ra)} calls on A, {len(rb)} on B; per call: rc | error text (where rc < 0) | values read back")
    diffs = abs(len(ra) - len(rb))
    for a, b in zip(ra, rb):
        same = a == b
        diffs += not same
        vals = "" if a[3] is None else f" | {len(a[3]) // 2} bytes" if isinstance(a[3], str) else \
            f" | {len(a[3])} values" if len(a[3]) > 8 or a[1] < 0 else " | " + " ".join(str(v) for v in a[3])
        print(f"{'same' if same else 'DIFF'}  {a[0]:<46} rc {a[1]:>3}{' | ' + a[2] if a[1] < 0 else ''}{vals}")
        if not same:
            print(f"      A: {a}\n      B: {b}")
    print(f"{diffs} differences")
    return diffs


def code_objects(path):
    """the gfx950 code objects of the clang offload bundles in the library's .hip_fatbin section -> [sha256] of the non-empty ones"""
    tmp = path + ".fatbin.tmp"
    objcopy = next(p for p in ("/opt/rocm/lib/llvm/bin/llvm-objcopy", "/usr/bin/objcopy") if os.path.exists(p))
    subprocess.run([objcopy, "-O", "binary", "--only-section=.hip_fatbin", path, tmp], check=True)
    blob = open(tmp, "rb").read()
    os.remove(tmp)
    magic, out, at = b"__CLANG_OFFLOAD_BUNDLE__", [], 0
    while (at := blob.find(magic, at)) >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(magic))
        p = at + len(magic) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                out.append(hashlib.sha256(blob[at + off:at + off + size]).hexdigest())
        at += len(magic)
    return out


def build_parent(rev="HEAD~1", where=os.path.join("build", "parent")):
    where = os.path.join(ROOT, where)
    os.makedirs(where, exist_ok=True)
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "gstreamer-vit-tracker_amd", "include", "harness"], capture_output=True, check=True).stdout
    subprocess.run(["tar", "-x", "-C", where], input=tar, check=True)
    subprocess.run([sys.executable, os.path.join(where, "gstreamer-vit-tracker_amd", "build.py")], check=True, stdout=subprocess.DEVNULL)
    print(os.path.join(where, "gstreamer-vit-tracker_amd", "libvittrack_hip.so"))


def objects(lib_a, lib_b):
    bad = 0
    sets = []
    for lib in (lib_a, lib_b):
        info = subprocess.run([sys.executable, "-c", "import ctypes,sys; l=ctypes.CDLL(sys.argv[1]); l.vt_build_info.restype=ctypes.c_char_p; print(l.vt_build_info().decode())",
                               os.path.abspath(lib)], capture_output=True, text=True, check=True).stdout.strip()
        objs = code_objects(lib)
        sets.append((info, collections.Counter(objs)))
        print(f"{lib}\n  vt_build_info: {info}\n  {len(objs)} non-empty gfx950 code objects")
        for h in sorted(objs):
            print(f"    {h}")
    bad += sets[0][0] != sets[1][0]
    bad += sets[0][1] != sets[1][1]
    print(f"build info {'the same' if sets[0][0] == sets[1][0] else 'DIFFERS'}; code objects {'the same multiset' if sets[0][1] == sets[1][1] else 'DIFFER'}")
    return bad


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        child()
    elif sys.argv[1:2] == ["--build-parent"] and len(sys.argv) <= 4:
        build_parent(*sys.argv[2:])
    elif len(sys.argv) == 4 and sys.argv[1] == "--objects":
        sys.exit(objects(sys.argv[2], sys.argv[3]))
    elif len(sys.argv) == 3:
        sys.exit(min(behaviour(sys.argv[1], sys.argv[2]), 1))
    else:
        sys.exit(__doc__)
