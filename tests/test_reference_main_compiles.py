"""The drop-in claim under test: the reference's OWN `main()` — the text of
src/common/bicg.cpp from `int main` to the end of the file, never stored here — compiles and links as written behind
`#include "mgs_host.hpp"` + `using namespace mgs;`.  build() compiles it by the recipe in oracle/Makefile into
oracle/_ref/ref_main_mgs (with its translation unit beside it) wherever the reference checkout was there to build from;
this test checks what that build made.  Only the usage path runs: no device is touched."""
import os
import subprocess

import pytest

from conftest import REPO

REF = os.path.join(REPO, "oracle", "_ref")
TU = os.path.join(REF, "ref_main_tu.cpp")
EXE = os.path.join(REF, "ref_main_mgs")


def test_reference_main_compiles_and_links_against_mgs_host():
    if not os.path.exists(os.path.join(REF, "ref_dump")):
        pytest.skip("oracle/_ref not built: the reference checkout was not there when build() ran")
    assert os.path.exists(TU) and os.path.exists(EXE), "oracle/_ref has the reference build but not ref_main_mgs (oracle/Makefile)"
    text = open(TU).read()
    assert '#include "mgs_host.hpp"' in text and "using namespace mgs;" in text
    main_src = text[text.index("int main"):]
    assert "BiCGSTABiml(A, x, b, precond, max_iter, tol)" in main_src and "readMatrix(" in main_src and "VectorXd" in main_src
    assert os.path.exists(os.path.join(REPO, "multigridsolver_amd", "libmgs.so")), "libmgs.so not built (run __graft_entry__.build())"
    # usage path (argc != 3) runs without a device: same message and exit code as the reference's main
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Incorrect number of arguments." in r.stdout
