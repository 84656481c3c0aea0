"""Host check (no GPU) of csrc/engine_registry.h, the parameter registry the three inference engines (dit.hip, uvit.hip, dit1d.hip) share:
tests/engine_registry_check.cpp is compiled with the host compiler alone -- the header takes no HIP header -- and run.  Its loaders only
record their calls.  What it checks: enumeration order, shapes up to 4 dimensions, the three refusals of load (null argument, unknown name,
wrong rank / extent) with each engine's message prefix, a loader's failure code passed through with the entry left unloaded, the first
missing entry in registration order, and a second load of one name running the loader again."""
import os
import shutil
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "diffusion-forcing-transformer_amd", "csrc")


def test_engine_registry(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (CXX, c++, g++, clang++)"
    exe = str(tmp_path / "engine_registry_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "engine_registry_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout == "ok\n", run.stdout + run.stderr

