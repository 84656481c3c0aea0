"""Host checks (no GPU) of csrc/dit_model.h, the one description of the DiT family both engines bind to: tests/dit_model_dump.cpp is compiled
with the host compiler and prints the inventory, the trainer's flat layout and the positional tables of an engine configuration.

  * names, order (and shapes, where recorded) against every list the fixtures recorded from the reference's own modules, the backbone
    configuration mapped to the engine's with the product's own DiT3D._configure / DifferenceDiT3D._configure on a bare instance;
  * the trainer's parameters = the inventory without the Fourier buffers, against the reference's lists of parameters with a gradient;
  * offsets: running sum of the element counts rounded up to 4; ldt / mod_final against the modulation rows the inventory lists;
  * the tables against float64 NumPy restatements of the reference's formulas (dit_base.py:527-572, embeddings.py:193-202,251-277).

Bars of the tables (derived, not measured).  Frequencies, sinusoidal_2d, the temporal table and the RoPE-1D are float64 expressions rounded
to fp32: one fp32 rounding of a value in [-1, 1], |delta| <= 2^-23.  The RoPE-3D works in fp32 like the reference: the angle carries at most
2 ulp of relative error (powf, the divide, the product; inv <= 1) and cosf / sinf about 1 ulp, |delta| <= 2^-21 * max(1, largest position).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dit_cond_common as dc
import dit_fac_common as fc
import dit_facmat_common as fm
from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "diffusion-forcing-transformer_amd", "csrc")
X_SHAPE, MAX_TOKENS = (4, 16, 8), 5  # 16 x 8 patches at patch 1: gh != gw, so the "xy" indexing of sinusoidal_2d shows
ACTION = dict(external_cond_type="action", external_cond_dim=3)
FOURIER = dict(use_fourier_noise_embedding=True)


def _facmat(tag, dropout=0.0):
    cc, rr, bias, ratio, rope = fm.CASES[tag]
    return fm.backbone_cfg(cc, rr, bias, ratio, rope, dropout)


# (fixture, key of the names, key of the shapes or None) -> (difference model, backbone configuration, constructor keywords)
STATE_DICTS = {
    ("dit_cond.npz", "act_d0_names", None): (False, dc.dit_cfg(0.0), ACTION),
    ("dit_cond.npz", "act_d1_names", None): (False, dc.dit_cfg(0.1), ACTION),
    ("dit_cond.npz", "label_names", None): (False, dc.dit_cfg(0.0), dict(external_cond_type="label", external_cond_num_classes=101, external_cond_dim=1)),
    ("dit_cond.npz", "diff_act_names", None): (True, dc.diff_cfg(0.1), ACTION),
    ("dit_cont.npz", "names", None): (False, {**dc.dit_cfg(), **FOURIER}, {}),
    ("dit_cont.npz", "act_names", None): (False, {**dc.dit_cfg(0.1), **FOURIER}, ACTION),
    ("dit_cont.npz", "diff_names", None): (True, {**dc.diff_cfg(), **FOURIER}, {}),
    ("dit_fac.npz", "names_mlp0", "shapes_mlp0"): (False, fc.backbone_cfg(0.0), {}),
    ("dit_fac.npz", "names_mlp4", "shapes_mlp4"): (False, fc.backbone_cfg(4.0), {}),
    ("dit_fac.npz", "names_act", "shapes_act"): (False, fc.backbone_cfg(0.0, fc.COND_DROPOUT), ACTION),
    **{("dit_facmat.npz", f"names_{t}", f"shapes_{t}"): (False, _facmat(t), {}) for t in fm.CASES},
    ("dit_facmat.npz", "names_act", "shapes_act"): (False, _facmat("a", fc.COND_DROPOUT), ACTION),
}
# the reference's parameters with a gradient (all of them): what the trainer's flat buffers hold
TRAINED = {
    ("dit_cont.npz", "train_dit_names"): (False, {**dc.dit_cfg(), **FOURIER}, {}),
    ("dit_cont.npz", "train_diff_names"): (True, {**dc.diff_cfg(), **FOURIER}, {}),
    ("dit_facmat_train.npz", "a_names"): (False, _facmat("a"), {}),
    ("dit_facmat_train.npz", "b_names"): (False, _facmat("b"), {}),
    ("training_grads.npz", "dit_names"): (False, dc.dit_cfg(), {}),
    ("training_grads.npz", "diff_names"): (True, dc.diff_cfg(), {}),
}


def engine_config(difference, cfg, external_cond_type="action", external_cond_num_classes=None, external_cond_dim=0):
    """what DiT3D.__init__ fills before it creates the engine, with the class's own _configure on a bare instance (no GPU)"""
    import dfot_amd
    from dfot_amd import capi, dit_backbone
    cls = dfot_amd.DifferenceDiT3D if difference else dfot_amd.DiT3D
    c = capi.DiTConfigF()
    c.depth, c.num_heads, c.patch_size = int(cfg["depth"]), int(cfg["num_heads"]), int(cfg["patch_size"])
    c.in_channels, c.height, c.width = X_SHAPE
    c.noise_dim, c.timesteps, c.rope_theta, c.eps = 256, 1000, 10000.0, 1e-6
    dit_backbone.configure_condition(c, cfg, external_cond_type, external_cond_num_classes, external_cond_dim)
    c.fourier_noise = int(bool(cfg.get("use_fourier_noise_embedding", False)))
    model = cls.__new__(cls)
    model.x_shape = X_SHAPE
    cls._configure(model, c, cfg, MAX_TOKENS)
    return {name: getattr(c, name) for name, _ in capi.DiTConfig._fields_ + capi.DiTConfigF._fields_}


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """compiles tests/dit_model_dump.cpp once; dump(fields) -> (geometry dict, inventory entries, directory of the tables)"""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (CXX, c++, g++, clang++)"
    work = tmp_path_factory.mktemp("dit_model")
    exe = str(work / "dit_model_dump")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "dit_model_dump.cpp"), "-o", exe], check=True)
    runs = {}

    def run(fields):
        key = tuple(sorted(fields.items()))
        if key not in runs:
            out = work / f"run{len(runs)}"
            out.mkdir()
            text = subprocess.run([exe, str(out)] + [f"{k}={v}" for k, v in fields.items()], check=True, capture_output=True, text=True).stdout
            head, *lines = text.splitlines()
            geom = {k: int(v) for k, v in (item.split("=") for item in head[2:].split())}
            entries = []
            for line in lines:
                name, *rest = line.split()
                n = next(i for i, tok in enumerate(rest) if tok.startswith("k"))
                block, temporal, buffer, col, offset = map(int, rest[n + 1:])
                entries.append(dict(name=name, shape=tuple(map(int, rest[:n])), kind=int(rest[n][1:]), block=block, temporal=bool(temporal),
                                    buffer=bool(buffer), col=col, offset=offset))
            runs[key] = (geom, entries, str(out))
        return runs[key]
    return run


def _names(fixture, key):
    return [str(n) for n in np.load(os.path.join(GOLDEN, fixture))[key]]


@pytest.mark.parametrize("fixture,key,shapes", list(STATE_DICTS), ids=[f"{f[:-4]}:{k}" for f, k, _ in STATE_DICTS])
def test_inventory_equals_the_reference_state_dict(dump, fixture, key, shapes):
    difference, cfg, kw = STATE_DICTS[fixture, key, shapes]
    _, entries, _ = dump(engine_config(difference, cfg, **kw))
    assert [e["name"] for e in entries] == _names(fixture, key)
    if shapes:
        assert [" ".join(map(str, e["shape"])) for e in entries] == _names(fixture, shapes)
    if "label" in key:  # the label table: num_classes rows, one more (the null class) with dropout
        table = next(e for e in entries if e["name"] == "external_cond_embedding.embedding_table.weight")
        assert table["shape"] == (101, 128) and dump(engine_config(difference, cfg, **kw))[0]["c_rows"] == 101
        geom, dropped, _ = dump(engine_config(difference, dc.dit_cfg(0.1), **kw))
        assert geom["c_rows"] == 102 and [e["name"] for e in dropped] == [e["name"] for e in entries]
        assert next(e for e in dropped if e["name"] == table["name"])["shape"] == (102, 128)
    else:
        assert dump(engine_config(difference, cfg, **kw))[0]["c_rows"] == 0
    buffers = [e["name"] for e in entries if e["buffer"]]
    assert buffers == ([n for n in _names(fixture, key) if ".timesteps." in n] if cfg.get("use_fourier_noise_embedding") else [])


@pytest.mark.parametrize("fixture,key", list(TRAINED), ids=[f"{f[:-4]}:{k}" for f, k in TRAINED])
def test_trainer_parameters_equal_the_reference_parameters(dump, fixture, key):
    difference, cfg, kw = TRAINED[fixture, key]
    _, entries, _ = dump(engine_config(difference, cfg, **kw))
    assert [e["name"] for e in entries if not e["buffer"]] == _names(fixture, key)
    assert len([e for e in entries if e["buffer"]]) == (2 if cfg.get("use_fourier_noise_embedding") else 0)


ALL_MODELS = list({**{k[:2]: v for k, v in STATE_DICTS.items()}, **TRAINED}.items())


@pytest.mark.parametrize("model", [v for _, v in ALL_MODELS], ids=[f"{f[:-4]}:{k}" for (f, k), _ in ALL_MODELS])
def test_flat_layout_and_modulation_columns(dump, model):
    difference, cfg, kw = model
    fields = engine_config(difference, cfg, **kw)
    geom, entries, _ = dump(fields)
    hidden = fields["hidden_size"]
    total = col = 0
    for e in entries:
        if e["buffer"]:
            assert e["offset"] == -1
            continue
        assert e["offset"] == total and total % 4 == 0
        total += -(-int(np.prod(e["shape"])) // 4) * 4
    assert geom["total"] == total
    bound = [(e["kind"], e["block"], e["temporal"]) for e in entries]
    assert len(set(bound)) == len(bound)  # what an engine binds storage by names every tensor once
    # every modulation Linear: weight and bias share the column, which is the running sum of the rows listed so far
    mods = [e for e in entries if ".modulation.1." in e["name"]]
    assert [e for e in entries if e["col"] >= 0] == mods and len(mods) % 2 == 0
    for w, b in zip(mods[0::2], mods[1::2]):
        final = w["name"].startswith("dit_base.final_layer.")
        rows = (2 if final else 3) * hidden
        assert w["name"].endswith(".weight") and b["name"] == w["name"][:-6] + "bias"
        assert w["shape"] == (rows, hidden) and b["shape"] == (rows,) and w["col"] == b["col"] == col
        if final:
            assert geom["mod_final"] == col and w is mods[-2]
        else:
            assert (".norm1." in w["name"] or ".norm2." in w["name"]) and w["block"] >= 0
        col += rows
    assert geom["ldt"] == col


# ---------------------------------------------------------------------------------------------------------------- the tables
def _table_fields(hidden=128, heads=4):
    return dict(hidden_size=hidden, depth=1, num_heads=heads, patch_size=1, in_channels=4, height=16, width=8, max_tokens=MAX_TOKENS, noise_dim=256,
                timesteps=1000, rope_theta=10000.0, num_row_heads=4)


def _table(directory, name, *shape):
    return np.fromfile(os.path.join(directory, name), dtype=np.float32).reshape(shape)


def _sincos(pos, n):
    """[sin | cos] of pos * 10000^(-i/n), float64"""
    ang = np.asarray(pos, dtype=np.float64)[:, None] / 10000.0 ** (np.arange(n, dtype=np.float64) / n)
    return np.concatenate([np.sin(ang), np.cos(ang)], axis=1)


def test_float64_tables(dump):
    fields = _table_fields()
    geom, _, out = dump(fields)
    gh, gw, hidden = 16, 8, 128
    assert (geom["gh"], geom["gw"], geom["P"]) == (gh, gw, gh * gw)
    bar = 2.0 ** -23
    half = fields["noise_dim"] // 2
    d = np.abs(_table(out, "freqs.f32", half) - np.exp(-np.log(10000.0) * np.arange(half) / half)).max()
    print(f"timestep frequencies: max |delta| {d:.1e}")
    assert d <= bar
    m = np.arange(gh * gw)  # meshgrid "xy": entry m takes m % gh for the first half of the channels, m // gh for the second
    want = np.concatenate([_sincos(m % gh, hidden // 4), _sincos(m // gh, hidden // 4)], axis=1)
    d = np.abs(_table(out, "pos2d.f32", gh * gw, hidden) - want).max()
    print(f"sinusoidal_2d: max |delta| {d:.1e}")
    assert d <= bar
    d = np.abs(_table(out, "tpos.f32", MAX_TOKENS, hidden) - _sincos(np.arange(MAX_TOKENS), hidden // 2)).max()
    print(f"temporal table: max |delta| {d:.1e}")
    assert d <= bar
    dim = hidden // fields["num_row_heads"]  # 4 row heads: 16 pairs per matrix row
    ang = np.arange(MAX_TOKENS, dtype=np.float64)[:, None] * 10000.0 ** (-2.0 * np.arange(dim // 2) / dim)
    d = np.abs(_table(out, "rope1d.f32", MAX_TOKENS, dim // 2, 2) - np.stack([np.cos(ang), np.sin(ang)], -1)).max()
    print(f"RoPE-1D: max |delta| {d:.1e}")
    assert d <= bar


@pytest.mark.parametrize("hidden,heads,head_dim", [(128, 4, 32), (128, 2, 64), (144, 2, 72)])  # (head_dim / 2) % 3 = 1, 2, 0
def test_rope_3d_table(dump, hidden, heads, head_dim):
    geom, _, out = dump(_table_fields(hidden, heads))
    gh, gw, half = 16, 8, head_dim // 2
    assert geom["d"] == head_dim
    q, rem = divmod(half, 3)
    parts = [q + (rem == 1), q + (rem == 2), q + (rem == 2)]  # RotaryEmbedding3D's split of the head dim over (t, h, w)
    tok = np.arange(MAX_TOKENS * gh * gw)
    pos = [tok // (gh * gw), (tok // gw) % gh, tok % gw]
    ang = np.concatenate([pos[ax][:, None] * 10000.0 ** (-2.0 * np.arange(parts[ax]) / (2 * parts[ax])) for ax in range(3)], axis=1)
    assert ang.shape == (len(tok), half)
    d = np.abs(_table(out, "rope3d.f32", len(tok), half, 2) - np.stack([np.cos(ang), np.sin(ang)], -1)).max()
    bar = 2.0 ** -21 * max(1, max(int(p.max()) for p in pos))
    print(f"RoPE-3D, head dim {head_dim}: max |delta| {d:.1e} (bar {bar:.1e})")
    assert d <= bar
