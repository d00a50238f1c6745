"""The programs of tests/cpp_face (one per family of multigridsolver_amd/cpp/mgs_host.hpp, run on the device by tests/test_gpu_cpp_face.py)
compile with -Wall and no warning, and each prints its usage and exits 1 before it touches a device."""
import os
import subprocess

import numpy as np
import pytest

import cpp_face


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    return cpp_face.compile_all(tmp_path_factory.mktemp("cpp_face_cpu"))


def test_one_program_per_family():
    sources = sorted(f[:-4] for f in os.listdir(cpp_face.SRC) if f.endswith(".cpp"))
    assert sources == sorted(cpp_face.FAMILIES)
    for fam in cpp_face.FAMILIES:
        text = open(os.path.join(cpp_face.SRC, fam + ".cpp")).read()
        assert "int main(" in text and "hip/" not in text, fam


@pytest.mark.parametrize("family", cpp_face.FAMILIES)
def test_usage_path_touches_no_device(exes, family):
    for args in ([], ["only_one"], ["a", "b", "c"]):
        r = subprocess.run([exes[family]] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stdout.startswith("usage:") and "IN_DIR OUT_DIR" in r.stdout, (family, args, r.returncode, r.stdout, r.stderr)


def test_the_helper_reads_what_the_programs_write(tmp_path):
    """the file formats of tests/cpp_face/face_io.hpp, written here by hand: %a scalars keep every bit, a name is never taken twice"""
    cpp_face.write_f64(tmp_path / "v.f64", [1.5, -0.0, np.nan])
    cpp_face.write_i32(tmp_path / "m.rp.i32", [0, 2, 3])
    (tmp_path / "scalars.txt").write_text("m.rows i 2\nresid d 0x1.999999999999ap-4\nneg d -0x0p+0\n")
    got = cpp_face.read_outputs(tmp_path)
    assert sorted(got) == ["m.rows", "m.rp", "neg", "resid", "v"]
    assert got["m.rows"] == 2 and got["resid"] == 0.1 and got["m.rp"].tolist() == [0, 2, 3]
    same = dict(got)
    cpp_face.compare(got, same)
    for name, other in (("neg", 0.0), ("resid", float(np.nextafter(0.1, 1.0))), ("m.rows", 3), ("v", np.array([1.5, 0.0, np.nan])), ("m.rp", np.array([0, 2], dtype=np.int32))):
        changed = dict(got); changed[name] = other
        with pytest.raises(AssertionError):
            cpp_face.compare(got, changed)
    missing = dict(got); del missing["v"]
    with pytest.raises(AssertionError):
        cpp_face.compare(got, missing)
