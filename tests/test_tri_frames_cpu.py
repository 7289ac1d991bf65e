"""Per-triangle shading frames (miw/shape.h: TriFrame, tri_frame, FaceNormalTable) on the CPU.

tools/tri_frames_check.cpp is a stand-alone program (its own main, the project's host flags): it runs a fixed list of triangles
— normals on each of the six axes, n.z == +0 and -0, slivers, coordinates of 1e-20 and 1e+15, zero-area triangles (a NaN frame),
each with and without vertex normals, with texture coordinates of zero and non-zero determinant — and 100 000 seeded random
triangles x 4 random hits through three routes: the statements of compute_surface_interaction as they stood before the split
(frozen in the program), the classic signature (tri_frame + the per-hit half) and the per-hit half alone over a table of
tri_frame() records built beforehand, which is what the packet kernels do in LDS. Every field of SurfaceInteraction is compared by
bit pattern (a NaN equals a NaN of any payload); the same for the forms of mesh_sample_position. Expected mismatches: 0.
The same program once more under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "tri_frames_check.cpp")


def _host_flags():
    from mitsuba2_amd import build
    return build.CXX, [f for f in build.CXX_FLAGS if f not in ("-fPIC", "-shared")]


pytestmark = pytest.mark.skipif(shutil.which(os.environ.get("CXX", "g++")) is None, reason="needs the host compiler")


def _build_and_run(tmp_path, name, extra, n_random, env=None):
    cxx, flags = _host_flags()
    exe = str(tmp_path / name)
    subprocess.check_call([cxx] + flags + extra + [SRC, "-o", exe])
    out = subprocess.run([exe, str(n_random)], capture_output=True, text=True, timeout=300, env=env)
    print(out.stdout, out.stderr[-2000:])
    return out


def test_frames_and_face_normals_reproduce_the_per_hit_code_bit_for_bit(tmp_path):
    out = _build_and_run(tmp_path, "tri_frames_check", [], 100000)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    assert "random triangles 100000," in out.stdout and "mismatches 0" in out.stdout.splitlines()[-1]


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    # (the sanitizer runtimes linked statically: the program needs nothing preloaded and asks nothing of what its environment preloads)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = _build_and_run(tmp_path, "tri_frames_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"], 100000, env=env)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    assert "mismatches 0" in out.stdout.splitlines()[-1] and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
