"""Repository contract checks that need no GPU: the C-ABI library loads and exports every declared symbol, the
product never imports the oracle, and the product has no CPU fallback."""
import ast
import ctypes
import os
import re

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "diffusion-forcing-transformer_amd")


def test_library_exports_every_symbol_declared_in_header():
    import __graft_entry__ as g
    g.build()
    hdr = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    declared = set(re.findall(r"\b(dfot_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 20
    lib = ctypes.CDLL(os.path.join(PKG, "libdfot_hip.so"))
    for name in sorted(declared):
        assert hasattr(lib, name), f"libdfot_hip.so does not export {name}"
    from dfot_amd import capi
    assert declared == set(capi.SIGNATURES), declared ^ set(capi.SIGNATURES)
    assert lib.dfot_version() >= 1


def test_gemm_descriptor_layout_matches_the_header():
    """capi.GemmDesc mirrors dfot_gemm_desc field by field: a field added, dropped or widened on one side only changes the size"""
    import __graft_entry__ as g
    g.build()
    from dfot_amd import capi
    assert ctypes.sizeof(capi.GemmDesc) == capi.lib.dfot_op_gemm_desc_bytes()


def _imports(path):
    tree = ast.parse(open(path).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            for a in node.names:
                yield a.name
        elif isinstance(node, ast.ImportFrom):
            yield ("." * node.level) + (node.module or "")


def test_product_never_imports_oracle_or_reference():
    for fn in os.listdir(PKG):
        if fn.endswith(".py"):
            for mod in _imports(os.path.join(PKG, fn)):
                assert not mod.lstrip(".").startswith("oracle"), f"{fn} imports {mod}"
                assert "reference" not in mod
    src = " ".join(open(os.path.join(PKG, "csrc", f)).read() for f in os.listdir(os.path.join(PKG, "csrc")))
    assert "/root/reference" not in src
    for fn in ("bench.py", "__graft_entry__.py"):
        assert "/root/reference" not in open(os.path.join(ROOT, fn)).read()


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location("capi_probe", os.path.join(PKG, "capi.py"))
    mod = importlib.util.module_from_spec(spec)
    real_exists = os.path.exists
    monkeypatch.setattr(os.path, "exists", lambda p: False if str(p).endswith("libdfot_hip.so") else real_exists(p))
    with pytest.raises(ImportError, match="no CPU fallback"):
        spec.loader.exec_module(mod)


def test_backbone_refuses_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import dfot_amd
    cfg = dict(channels=[128, 256, 576, 1152], emb_channels=1024, num_updown_blocks=[1, 1, 1], num_mid_blocks=1,
               num_heads=9, conditioning=dict(dim=180))
    with pytest.raises(dfot_amd.capi.DfotError):
        dfot_amd.UViT3DPose(cfg, x_shape=(3, 64, 64), max_tokens=8)


def test_torch_library_operators_are_registered_with_shape_inference():
    """The engine's entry points are torch operators (namespace dfot) with fake implementations: FakeTensor tracing works
    without a GPU and without touching the HIP library."""
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    import dfot_amd  # noqa: F401  (registers the operators)
    for name in ("uvit3d_pose_forward", "dit3d_forward", "ray_encoding", "hg_prepare", "ddim_hg_step"):
        assert hasattr(torch.ops.dfot, name), name
    with FakeTensorMode():
        enc = torch.ops.dfot.ray_encoding(torch.empty(2, 8, 16), 64)
        assert tuple(enc.shape) == (2, 8, 180, 64, 64)
        x = torch.empty(2, 8, 3, 64, 64)
        v = torch.ops.dfot.uvit3d_pose_forward(x, torch.empty(2, 8), enc, None, 0)
        assert v.shape == x.shape
        x_in = torch.ops.dfot.hg_prepare(x, None, torch.empty(4, 8), torch.empty(4, 8), 2)
        assert tuple(x_in.shape) == (4, 8, 3, 64, 64)
        nxt = torch.ops.dfot.ddim_hg_step(x, x_in, x_in, *(torch.empty(4, 8) for _ in range(5)), torch.empty(2), torch.empty(2, 8, dtype=torch.uint8), 2)
        assert nxt.shape == x.shape
        z = torch.empty(3, 5, 16, 16, 16)
        assert torch.ops.dfot.dit3d_forward(z, torch.empty(3, 5, dtype=torch.long), 0).shape == z.shape


def test_no_kernel_spills_registers(tmp_path):
    """Every gfx950 kernel must fit its register budget: a refactor once wrapped the 16-wave GEMM kernels (128-VGPR cap) in a
    tile loop and silently spilled up to 35 VGPRs, 20 % of the fused QKV GEMM's time.  Compiles each source to ISA (no GPU
    needed) and reads the code-object metadata."""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not shutil.which(hipcc) and not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(PKG, "csrc")
    offenders = []
    procs = []
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith(".hip"):
            continue
        out = tmp_path / (fn + ".s")
        procs.append((fn, out, subprocess.Popen(
            [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-I", os.path.join(ROOT, "include"),
             "-I", csrc, "--offload-device-only", "-S", "-o", str(out), os.path.join(csrc, fn)],
            stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)))
    for fn, out, p in procs:
        assert p.wait() == 0, f"{fn} failed to compile"
        text = open(out).read()
        names = re.findall(r"\.name:\s+(\S+)", text)
        spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)
        assert spills, fn
        for m in re.finditer(r"\.name:\s+(\S+)(.*?)\.wavefront_size", text, re.S):
            sp = re.search(r"\.vgpr_spill_count:\s+(\d+)", m.group(2))
            if sp and int(sp.group(1)) > 0:
                offenders.append((fn, m.group(1)[:80], int(sp.group(1))))
        assert names
    assert not offenders, offenders


def _header_prototypes():
    """name -> (return type, [argument declarations]) of every function include/dfot_hip.h declares (comments stripped)"""
    hdr = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?\**)\s*\b(dfot_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, re.S):
        args = " ".join(m.group(3).split())
        protos[m.group(2)] = (" ".join(m.group(1).split()), [] if args in ("", "void") else [a.strip() for a in args.split(",")])
    return protos


def _ctype_of(decl):
    """the ctypes class a C declaration ("const float* x", "int64_t n", "dfot_uvit_t h", "const char*") must be bound with; 'ptr' for any pointer
    (array parameters included)"""
    words = decl.replace("*", " * ").split()
    if "*" in words or "[" in decl or words[0].endswith("_t") and words[0].startswith("dfot_"):  # the handle typedefs are struct pointers
        return "ptr"
    base = [w for w in words if w not in ("const", "unsigned")]
    return {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
            "size_t": ctypes.c_size_t}[base[0]]


def _is_pointer_ctype(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def test_ctypes_signatures_match_the_header_prototypes_argument_by_argument():
    """capi.SIGNATURES binds every entry point with the header's argument list: same count, int -> c_int, int64_t -> c_int64, float ->
    c_float, size_t -> c_size_t, any pointer -> c_void_p / c_char_p / POINTER.  A mismatch passes garbage through ctypes silently
    (an int64_t bound as c_int truncates; a float bound as c_int reinterprets)."""
    from dfot_amd import capi
    protos = _header_prototypes()
    assert set(protos) == set(capi.SIGNATURES), set(protos) ^ set(capi.SIGNATURES)
    bad = []
    for name, (ret, args) in sorted(protos.items()):
        res, argtypes = capi.SIGNATURES[name]
        if len(args) != len(argtypes):
            bad.append(f"{name}: {len(args)} arguments in the header, {len(argtypes)} bound")
            continue
        for i, (decl, bound) in enumerate(zip(args + [ret], list(argtypes) + [res])):
            want = _ctype_of(decl)
            ok = _is_pointer_ctype(bound) if want == "ptr" else bound is want
            if not ok:
                bad.append(f"{name} {'return' if i == len(args) else f'argument {i}'} `{decl}` bound as {getattr(bound, '__name__', bound)}")
    assert not bad, "\n".join(bad)


def test_every_op_entry_point_is_named_by_a_test():
    """every dfot_op_* symbol of the header is called (named) in at least one tests/test_*.py file: a new entry point cannot land untested"""
    names = sorted(n for n in _header_prototypes() if n.startswith("dfot_op_"))
    assert len(names) >= 60
    tdir = os.path.join(ROOT, "tests")
    text = "\n".join(open(os.path.join(tdir, f)).read() for f in sorted(os.listdir(tdir)) if f.startswith("test_") and f.endswith(".py"))
    untested = [n for n in names if not re.search(r"\b" + n + r"\b", text)]
    assert not untested, untested
