"""CPU-side checks of the boundary: libnslam.so loads, exports every symbol include/nslam.h
declares, and the Python pack layout agrees with the C++ one (no GPU calls)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO


def _header_symbols():
    txt = open(os.path.join(REPO, "include", "nslam.h")).read()
    return sorted(set(re.findall(r"\b(nslam_[a-z_0-9]+)\s*\(", txt)))


def test_library_exports_every_header_symbol(pkg):
    L = pkg._lib.lib()
    syms = _header_symbols()
    assert len(syms) >= 10
    for name in syms:
        assert hasattr(L, name), f"libnslam.so does not export {name}"
    assert set(syms) == set(pkg._lib.EXPORTS)


def test_abi_version_and_strerror(pkg):
    L = pkg._lib.lib()
    assert L.nslam_abi_version() == pkg._lib.ABI_VERSION == 24
    assert L.nslam_strerror(0) == b"ok"
    assert b"invalid" in L.nslam_strerror(-1)


def test_pack_layout_matches_python(pkg):
    P = pkg.packing
    for nc in (1, 2):
        c = pkg._lib.pack_layout(0, nc)
        py = P.xyz_layout(nc)
        assert c["total"] == py["total"] and c["vec"] == py["V"]
        assert c["nf"] == py["nf"] and c["nb"] == py["nfrag"] - py["nf"]
    c = pkg._lib.pack_layout(1, 1)
    py = P.noxyz_layout()
    assert c["total"] == py["total"] and c["vec"] == py["V"] and c["nf"] == py["nf"]


def test_argument_validation_without_gpu(pkg):
    """Entry points reject bad arguments before touching the device."""
    L = pkg._lib.lib()
    cfg = pkg._lib.NslamQueryCfg()
    cfg.stage = 7
    assert L.nslam_query_fwd(ctypes.byref(cfg), None, 10, None, None) == -1
    assert L.nslam_query_bwd(ctypes.byref(cfg), None, 10, None, None, None, 0, None) == -1
    assert L.nslam_composite_fwd(None, None, 4, 0, None, None, None, None) == -1
    assert L.nslam_composite_fwd(None, None, 4, 1000, None, None, None, None) == -2
    dims = (ctypes.c_int32 * 3)(0, 1, 1)
    assert L.nslam_grid_sample_fwd(None, dims, None, 5, None, None) == -1
    lo = (ctypes.c_double * 3)(0, 0, 0)
    assert L.nslam_sample_rays(None, None, None, None, 3, lo, lo, None, 500, None, 0, 0, None, None, 0, None) == -2
    assert L.nslam_rows_pack(None, None, 4, 30, None, 0, None, None) == -1      # row_len % 4
    assert L.nslam_rows_pack(None, None, 4, 32, None, 0, None, None) == -1      # NULL grid/rows
    assert L.nslam_rows_unpack(None, None, 0, 32, None, None, 5, None) == -1    # NULL tail
    assert L.nslam_rows_pack(None, None, 0, 32, None, 0, None, None) == 0       # empty: no launch


def test_no_cpu_fallback(pkg):
    import torch
    with pytest.raises(RuntimeError, match="HIP device"):
        pkg.ops.composite(torch.zeros(2, 4, 4), torch.zeros(2, 4, dtype=torch.float64))


# the C name(s) of every ctypes mirror in _lib.py (nslam_imap_grads has nslam_imap_params' layout and one mirror)
_C_STRUCTS = {
    "NslamGrid": ("nslam_grid",), "NslamDecGrad": ("nslam_dec_grad",), "NslamQueryCfg": ("nslam_query_cfg",),
    "NslamFrame": ("nslam_frame",), "NslamLossCfg": ("nslam_loss_cfg",), "NslamAdamSeg": ("nslam_adam_seg",),
    "NslamDraw": ("nslam_draw",), "NslamCamTail": ("nslam_cam_tail",), "NslamCamTailLr2": ("nslam_cam_tail_lr2",),
    "NslamImapParams": ("nslam_imap_params", "nslam_imap_grads"), "NslamImapQuery": ("nslam_imap_query",),
}


def _run_probe(tmp_path, statements):
    """Compile the statements as the body of a C main that includes nslam.h (gcc), run it → its output lines."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nslam.h"', "int main(void) {"]
    lines += list(statements) + ["  return 0; }"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    return [l for l in out if l]


def test_struct_layouts_match_header(pkg, tmp_path):
    """sizeof/offsetof of every ABI struct, compiled by gcc from include/nslam.h, equal the ctypes
    mirrors in _lib.py: every ctypes.Structure the module defines, under each C name it mirrors."""
    L = pkg._lib
    mirrors = {n: c for n, c in vars(L).items() if isinstance(c, type) and issubclass(c, ctypes.Structure)
               and c.__module__ == L.__name__}
    assert set(mirrors) == set(_C_STRUCTS), "a ctypes mirror in _lib.py without its C name here (or the reverse)"
    structs = {cname: mirrors[n] for n, cnames in _C_STRUCTS.items() for cname in cnames}
    assert len(structs) == 12 and {"nslam_grid", "nslam_dec_grad", "nslam_query_cfg", "nslam_frame", "nslam_loss_cfg",
                                   "nslam_adam_seg", "nslam_draw"} <= set(structs)
    header = open(os.path.join(REPO, "include", "nslam.h")).read()
    assert set(re.findall(r"^\} *(nslam_\w+);", header, re.M)) == set(structs)  # every struct typedef of the header
    lines = []
    for cname, py in structs.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in _run_probe(tmp_path, lines)}
    for cname, py in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(py), cname
        for f in py._fields_:
            assert got[(cname, f[0])] == getattr(py, f[0]).offset, (cname, f[0])


def test_every_export_has_a_declared_signature(pkg):
    """After lib() has bound, every export has argtypes set (nslam_abi_version takes none): an export without
    them would be called with ctypes' default conversions."""
    L = pkg._lib.lib()
    for name in pkg._lib.EXPORTS:
        if name != "nslam_abi_version":
            assert getattr(L, name).argtypes is not None, name


def _header_text():
    """include/nslam.h without its comments."""
    txt = open(os.path.join(REPO, "include", "nslam.h")).read()
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", txt, flags=re.S))


def _header_prototypes():
    """Every top-level prototype `ret nslam_name(params);` of the header (several lines, or `void`, included) →
    [(name, ret, [(base type, pointer depth), ...])].  const and a leading struct are dropped; `name[3]` is a
    pointer; ret keeps its stars ("const char*" → "char*")."""
    def ctype(text):
        words = [w for w in text.replace("*", " ").split() if w not in ("const", "struct")]
        return " ".join(words), text.count("*")

    protos = []
    prototype = r"^([A-Za-z_][\w \t*]*?)\b(nslam_\w+)\s*\(([^()]*)\)\s*;"
    for ret, name, params in re.findall(prototype, _header_text(), re.M):
        args = []
        for p in (() if params.strip() == "void" else params.split(",")):
            text, _, array = re.fullmatch(r"\s*(.*?)(\w+)\s*(\[\w*\])?\s*", p, re.S).groups()
            base, depth = ctype(text)
            args.append((base, depth + (1 if array else 0)))
        base, depth = ctype(ret)
        protos.append((name, base + "*" * depth, args))
    return protos


_C_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
              "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}
_C_POINTEES = dict(_C_SCALARS, int8_t=ctypes.c_int8, uint8_t=ctypes.c_uint8, int16_t=ctypes.c_int16,
                   uint16_t=ctypes.c_uint16, uint32_t=ctypes.c_uint32)
_C_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64, "char*": ctypes.c_char_p}


def _signature_faults(protos, table, mirrors):
    """Where table (name → (restype, argtypes)) departs from the prototypes → [(name, argument index or "restype" or
    "count", what)].  A scalar must be the ctypes class of exactly its C type; a pointer may be c_void_p or POINTER
    of its pointee's class; a struct pointer must be POINTER of the struct's mirror (mirrors: C name → class), a
    pointer to pointer c_void_p or POINTER(c_void_p); restype is exact; no entry point is exempt."""
    faults = []
    for name, ret, args in protos:
        if name not in table:
            faults.append((name, "count", "not in the table"))
            continue
        restype, argtypes = table[name]
        if restype is not _C_RETURNS.get(ret):
            faults.append((name, "restype", f"{ret} bound as {restype}"))
        if len(argtypes) != len(args):
            faults.append((name, "count", f"{len(args)} parameters, {len(argtypes)} argtypes"))
            continue
        for i, ((base, depth), got) in enumerate(zip(args, argtypes)):
            if depth == 0:
                allowed = [_C_SCALARS.get(base)]
            elif depth == 2:
                allowed = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
            elif depth == 1 and base in mirrors:
                allowed = [ctypes.POINTER(mirrors[base])]
            elif depth == 1 and base in _C_POINTEES:
                allowed = [ctypes.c_void_p, ctypes.POINTER(_C_POINTEES[base])]
            else:
                allowed = [ctypes.c_void_p] if (depth, base) == (1, "void") else []  # an unknown type matches nothing
            if not any(got is a for a in allowed):
                faults.append((name, i, f"{base}{'*' * depth} bound as {got}"))
    return faults


def test_signatures_match_header(pkg):
    """restype and every argtype of _lib.SIGNATURES against the prototypes of include/nslam.h (_signature_faults has
    the rule): all 91 entry points, none left out.  The same comparison then runs on a copy of the table with two
    planted faults (a c_float for nslam_mesh_select's double threshold, argument 5 counted from 0; a c_int32 for
    nslam_query_fwd's int64_t n_pts, argument 2) and must report exactly those, by name and index."""
    lib = pkg._lib
    mirrors = {cname: getattr(lib, py) for py, cnames in _C_STRUCTS.items() for cname in cnames}
    protos = _header_prototypes()
    names = [p[0] for p in protos]
    assert len(set(names)) == len(names)
    assert len(protos) == len(_header_symbols()) == len(lib.SIGNATURES) == 91
    assert names == list(lib.SIGNATURES), "SIGNATURES is kept in the header's order"
    faults = _signature_faults(protos, lib.SIGNATURES, mirrors)
    print(f"{len(protos)} prototypes compared, {len(faults)} faults")
    assert faults == []

    planted = {n: (r, list(a)) for n, (r, a) in lib.SIGNATURES.items()}
    assert planted["nslam_mesh_select"][1][5] is ctypes.c_double and planted["nslam_query_fwd"][1][2] is ctypes.c_int64
    planted["nslam_mesh_select"][1][5] = ctypes.c_float
    planted["nslam_query_fwd"][1][2] = ctypes.c_int32
    caught = _signature_faults(protos, planted, mirrors)
    print(f"planted faults caught: {caught}")
    assert [(n, i) for n, i, _ in caught] == [("nslam_query_fwd", 2), ("nslam_mesh_select", 5)]


# the enumerator families of nslam.h that the Python side uses: _lib.py mirrors each completely
_C_FAMILIES = {"error code": r"NSLAM_(OK|E[A-Z]+)", "stage": r"NSLAM_STAGE_\w+", "decoder": r"NSLAM_DEC_\w+",
               "loss mode": r"NSLAM_LOSS_\w+", "cull mode": r"NSLAM_CULL_\w+", "raster flag": r"NSLAM_RASTER_\w+",
               "scene flag": r"NSLAM_SCENE_\w+"}


def _mirror(lib, cname):
    """The value _lib.py holds for the header's NSLAM_X: _lib.NSLAM_X or _lib.X, a stage in STAGES and a cull mode in
    CULL_MODES under its lower-case name; None when _lib.py has none."""
    short = cname[len("NSLAM_"):]
    for prefix, table in (("STAGE_", lib.STAGES), ("CULL_", lib.CULL_MODES)):
        if short.startswith(prefix):
            return table.get(short[len(prefix):].lower())
    return getattr(lib, cname, getattr(lib, short, None))


def test_named_constants_match_header(pkg, tmp_path):
    """Every `#define NSLAM_*` with a numeric value and every enumerator of include/nslam.h, printed by a gcc
    probe: each one _lib.py mirrors is equal, the enumerator families the Python side uses are mirrored
    completely, and the names the rest of the package re-exports are those values."""
    lib, txt = pkg._lib, _header_text()
    defines = [n for n, v in re.findall(r"^#define[ \t]+(NSLAM_\w+)[ \t]+(\S.*)$", txt, re.M)
               if re.fullmatch(r"[\d\s()*+<-]+", v)]
    enumerators = [item.split("=")[0].strip() for body in re.findall(r"\benum\b[^{;]*\{([^}]*)\}", txt)
                   for item in body.split(",") if item.strip()]
    assert {"NSLAM_EMB", "NSLAM_MAX_FRAMES", "NSLAM_ADAM_MAX_SEGS", "NSLAM_CAM_GRAD_WS_DOUBLES"} <= set(defines)
    assert len(enumerators) == len(set(enumerators)) >= 20 and all(re.fullmatch(r"NSLAM_\w+", e) for e in enumerators)
    out = _run_probe(tmp_path, [f'  printf("{n} %lld\\n", (long long)({n}));' for n in defines + enumerators])
    value = {l.split()[0]: int(l.split()[1]) for l in out}
    assert set(value) == set(defines + enumerators)

    mirrored = {n: _mirror(lib, n) for n in value if _mirror(lib, n) is not None}
    for n, v in mirrored.items():
        assert v == value[n], (n, v, value[n])
    assert {"NSLAM_EMB", "NSLAM_MAX_FRAMES", "NSLAM_ADAM_MAX_SEGS", "NSLAM_CAM_GRAD_WS_DOUBLES"} <= set(mirrored)
    for family, pattern in _C_FAMILIES.items():
        members = [n for n in enumerators if re.fullmatch(pattern, n)]
        assert members and set(members) <= set(mirrored), (family, sorted(set(members) - set(mirrored)))
    # the two dicts hold nothing the header lacks
    assert len(lib.STAGES) == sum(n.startswith("NSLAM_STAGE_") for n in enumerators)
    assert len(lib.CULL_MODES) == sum(n.startswith("NSLAM_CULL_") for n in enumerators)
    # the public names elsewhere in the package are these values, not copies
    ops = pkg.ops
    assert ops.CAM_GRAD_WS_DOUBLES == value["NSLAM_CAM_GRAD_WS_DOUBLES"] and ops.CULL_MODES is lib.CULL_MODES
    assert (ops.RASTER_CLEAR, ops.RASTER_SMALL, ops.RASTER_BIG, ops.RASTER_RESOLVE, ops.RASTER_ALL) == tuple(
        value["NSLAM_RASTER_" + n] for n in ("CLEAR", "SMALL", "BIG", "RESOLVE", "ALL"))
    assert (ops.SCENE_POINTS, ops.SCENE_ALL) == (value["NSLAM_SCENE_POINTS"], value["NSLAM_SCENE_ALL"])
    assert pkg.packing.EMB == value["NSLAM_EMB"] and pkg.tsdf.MAX_FRAMES == lib.MAX_FRAMES == value["NSLAM_MAX_FRAMES"]


def test_v4_entry_points_validate_without_gpu(pkg):
    L = pkg._lib.lib()
    lib = pkg._lib
    fr = (lib.NslamFrame * 1)()
    assert L.nslam_gather_rays(fr, 0, 10, None, 10, 10, 0, 10, 0, 10, 1.0, 1.0, 0.0, 0.0, None, None,
                               None, None, None, None, None, None, None, None) == -1
    assert L.nslam_gather_rays(fr, 1, 10, None, 10, 10, 0, 11, 0, 10, 1.0, 1.0, 0.0, 0.0, None, None,
                               None, None, None, None, None, None, None, None) == -1
    # ABI v7: neither pix nor draws, and draws without device counter/ticket, are rejected
    fr[0].depth = fr[0].color = fr[0].c2w = 64
    assert L.nslam_gather_rays(fr, 1, 10, None, 10, 10, 0, 10, 0, 10, 1.0, 1.0, 0.0, 0.0, None, None,
                               64, 64, 64, 64, None, None, None, None) == -1
    draw = lib.NslamDraw(7, None, None)
    assert L.nslam_gather_rays(fr, 1, 10, None, 10, 10, 0, 10, 0, 10, 1.0, 1.0, 0.0, 0.0, None, None,
                               64, 64, 64, 64, None, ctypes.byref(draw), None, None) == -1
    cfg = lib.NslamLossCfg(5, 0, 0, 0.2)
    assert L.nslam_render_loss(ctypes.byref(cfg), None, None, 4, 48, None, None, None, None, None, None, None,
                               None, None, 0, None) == -1
    cfg = lib.NslamLossCfg(lib.LOSS_MAPPER, 0, 0, 0.2)
    assert L.nslam_render_loss(ctypes.byref(cfg), None, None, 4, 1000, None, None, None, None, None, None, None,
                               None, None, 0, None) == -2
    cfg = lib.NslamLossCfg(lib.LOSS_TRACKER, 1, 1, 0.5)
    assert L.nslam_render_loss_workspace_size(ctypes.byref(cfg), 100) == 101 * 8
    seg = (lib.NslamAdamSeg * 1)()
    assert L.nslam_adam_step(seg, 0, 0.9, 0.999, 1e-8, 1, None, None) == -1
    seg[0].n, seg[0].rows, seg[0].row_len = 4, 16, 6   # row_len % 4 != 0
    for f in ("param", "grad", "exp_avg", "exp_avg_sq", "step"):
        setattr(seg[0], f, 64)
    assert L.nslam_adam_step(seg, 1, 0.9, 0.999, 1e-8, 1, 64, None) == -1


def test_v8_cam_grad_validates_without_gpu(pkg):
    L = pkg._lib.lib()
    assert L.nslam_cam_grad(None, 64, 64, 64, 64, 10, 48, 64, None) == -1   # no cam
    assert L.nslam_cam_grad(64, 64, 64, 64, 64, -1, 48, 64, None) == -1     # negative ray count
    assert L.nslam_cam_grad(64, 64, None, 64, 64, 10, 48, 64, None) == -1   # rays without g_pts
    assert L.nslam_cam_grad(64, 64, 64, 64, 64, 10, 0, 64, None) == -1      # no samples
    # g_pts rows are indexed p*3+k in 32 bits: 3 * rays * samples must stay below 2^31
    assert L.nslam_cam_grad(64, 64, 64, 64, 64, (1 << 31) // 3 // 48 + 1, 48, 64, None) == -2


def test_v8_cam_pose_validates_without_gpu(pkg):
    L = pkg._lib.lib()
    assert L.nslam_cam_pose(None, 64, None) == -1
    assert L.nslam_cam_pose(64, None, None) == -1


def _colour_cfg(pkg):
    """A colour-stage config with fake (aligned, never dereferenced) device pointers: the entry points
    below must reject or accept it from the arguments alone, before any launch."""
    cfg = pkg._lib.NslamQueryCfg()
    cfg.stage = pkg._lib.STAGES["color"]
    for d in range(4):
        cfg.grid[d].data = 4096
        cfg.grid[d].dims[0] = cfg.grid[d].dims[1] = cfg.grid[d].dims[2] = 8
        cfg.packed[d] = 4096
    return cfg


def test_v16_bwd_decoders_validates_without_gpu(pkg):
    """nslam_query_bwd_decoders rejects bad configs, masks and parameter gradients before any launch."""
    L = pkg._lib.lib()
    cfg = pkg._lib.NslamQueryCfg()
    cfg.stage = 7
    gps = (ctypes.c_void_p * 4)()
    assert L.nslam_query_bwd_decoders(ctypes.byref(cfg), 0b0110, None, 10, None, gps, None) == -1  # stage
    ok = pkg._lib.NslamQueryCfg()
    rc = L.nslam_query_bwd_decoders(ctypes.byref(ok), 0, None, 0, None, gps, None)
    assert rc < 0  # an empty decoder mask (or an otherwise incomplete config) is never launched
    c = _colour_cfg(pkg)
    c.dgrad[pkg._lib.DEC_COLOR].base = 4096
    c.dgrad[pkg._lib.DEC_COLOR].count = 100
    colour = 1 << pkg._lib.DEC_COLOR
    # no parameter gradients in the lean launch (v16: the colour decoder's come from nslam_color_wgrad)
    assert L.nslam_query_bwd_decoders(ctypes.byref(c), colour, 4096, 10, 4096, gps, None) == -2
    c.dgrad[pkg._lib.DEC_COLOR].base = None
    assert L.nslam_query_bwd_decoders(ctypes.byref(c), colour, 4096, 10, 4096, gps, None) == -2  # no saved masks
    assert L.nslam_query_bwd_decoders(ctypes.byref(c), 1 << pkg._lib.DEC_COARSE, 4096, 10, 4096, gps, None) == -1


def test_v16_color_wgrad_validates_without_gpu(pkg):
    """nslam_color_wgrad rejects configs without a colour weight-gradient tape backward, a missing
    cotangent and a short workspace before any launch; an empty batch is a no-op."""
    L = pkg._lib.lib()
    cfg = pkg._lib.NslamQueryCfg()
    cfg.stage = 7
    assert L.nslam_color_wgrad(ctypes.byref(cfg), None, 10, None, None, 0, None) == -1            # bad stage
    c = _colour_cfg(pkg)
    c.stage = pkg._lib.STAGES["middle"]
    assert L.nslam_color_wgrad(ctypes.byref(c), 4096, 10, 4096, 4096, 1 << 20, None) == -1        # not colour
    c.stage = pkg._lib.STAGES["color"]
    assert L.nslam_color_wgrad(ctypes.byref(c), 4096, 10, 4096, 4096, 1 << 20, None) == -2        # no dgrad
    c.dgrad[pkg._lib.DEC_COLOR].base = 4096
    c.dgrad[pkg._lib.DEC_COLOR].count = 15575
    assert L.nslam_color_wgrad(ctypes.byref(c), 4096, 10, 4096, 4096, 1 << 20, None) == -2        # no tapes
    c.act_tape = 4096
    c.saved_masks = 4096
    assert L.nslam_color_wgrad(ctypes.byref(c), 4096, 10, None, 4096, 1 << 20, None) == -1        # no g_raw
    assert L.nslam_color_wgrad(ctypes.byref(c), None, 10, 4096, 4096, 1 << 20, None) == -1        # no points
    need = L.nslam_query_bwd_decoder_workspace_size(ctypes.byref(c), pkg._lib.DEC_COLOR, 10)
    assert need > 0
    assert L.nslam_color_wgrad(ctypes.byref(c), 4096, 10, 4096, 4096, need - 1, None) == -3       # short ws
    assert L.nslam_color_wgrad(ctypes.byref(c), 4096, 10, 4096, None, need, None) == -3           # no ws
    assert L.nslam_color_wgrad(ctypes.byref(c), None, 0, None, None, 0, None) == 0                # empty batch


def test_v16_removed_entry_points(pkg):
    """ABI v16 dropped the options measured neutral or slower in round 3 (the fused colour Adam, the
    part-wise forward of the pipelined loop), and ABI v24 dropped nslam_track_best (superseded by
    nslam_loss_sum_best and nslam_cam_grad_step, no caller left): they are no longer exported."""
    L = pkg._lib.lib()
    for name in ("nslam_color_wgrad_adam", "nslam_query_fwd_parts", "nslam_track_best"):
        assert not hasattr(L, name), name


def test_v15_cam_grad_parts_validates_without_gpu(pkg):
    """nslam_cam_grad_parts rejects missing buffers, bad part counts and oversized point counts."""
    L = pkg._lib.lib()
    bufs = (ctypes.c_void_p * 4)(64, 64, 64, 64)
    assert L.nslam_cam_grad_parts(64, 64, bufs, 3, 64, 64, 10, 48, 64, None, 64, None) == -1       # no ws
    assert L.nslam_cam_grad_parts(64, 64, bufs, 3, 64, 64, 10, 48, 64, 64, None, None) == -1       # no ticket
    assert L.nslam_cam_grad_parts(64, 64, bufs, 0, 64, 64, 10, 48, 64, 64, 64, None) == -1         # no parts
    assert L.nslam_cam_grad_parts(64, 64, bufs, 5, 64, 64, 10, 48, 64, 64, 64, None) == -1         # too many
    bufs[1] = None
    assert L.nslam_cam_grad_parts(64, 64, bufs, 3, 64, 64, 10, 48, 64, 64, 64, None) == -1         # a NULL part
    bufs[1] = 64
    assert L.nslam_cam_grad_parts(64, 64, bufs, 3, 64, 64, (1 << 31) // 3 // 48 + 1, 48, 64, 64, 64, None) == -2


def test_v19_cam_batch_validates_without_gpu(pkg):
    """nslam_cam_grad_batch / nslam_cam_pose_batch reject bad camera counts, strides, buffers and ray slices
    outside the batch before any launch."""
    L = pkg._lib.lib()
    bufs = (ctypes.c_void_p * 4)(64, 64, 64, 64)
    rb = (ctypes.c_int64 * 2)(0, 100)
    args = lambda **k: dict(dict(cams=64, c2w=64, stride=16, n=2, rb=rb, per=100, bufs=bufs, parts=3, z=64, rd=64,  # noqa: E731
                                 N=200, S=48, out=64, ws=64, tk=64), **k)

    def call(a):
        return L.nslam_cam_grad_batch(a["cams"], a["c2w"], a["stride"], a["n"], a["rb"], a["per"], a["bufs"],
                                      a["parts"], a["z"], a["rd"], a["N"], a["S"], a["out"], a["ws"], a["tk"], None)
    assert call(args(n=0)) == -1                       # no cameras
    assert call(args(n=33)) == -1                      # more than NSLAM_MAX_FRAMES
    assert call(args(stride=8)) == -1                  # a c2w stride shorter than a [3,4] pose
    assert call(args(tk=None)) == -1                   # no tickets
    assert call(args(ws=None)) == -1                   # no workspace
    assert call(args(parts=5)) == -1                   # too many d/dpts parts
    assert call(args(per=101)) == -1                   # camera 1's slice ends past the batch
    assert call(args(rb=None)) == -1                   # no slice table
    assert call(args(N=(1 << 31) // 3 // 48 + 1, per=100)) == -2
    assert L.nslam_cam_pose_batch(None, 64, 16, 2, None) == -1
    assert L.nslam_cam_pose_batch(64, 64, 16, 0, None) == -1
    assert L.nslam_cam_pose_batch(64, 64, 8, 2, None) == -1


def test_v20_frustum_rows_validates_without_gpu(pkg):
    L = pkg._lib.lib()
    need = L.nslam_frustum_rows_workspace_size(10 * 12 * 20)
    assert need > 2400 * 5 and L.nslam_frustum_rows_workspace_size(0) == 0
    args = [64, 64, 64, 680, 1200, 20, 12, 10, 64, 64, 64, None, 64, need, None]
    for i in (0, 1, 2, 8, 9, 10):  # a missing input / output buffer
        a = list(args)
        a[i] = None
        assert L.nslam_frustum_rows(*a) == -1, i
    a = list(args)
    a[5] = 0                            # an empty grid axis
    assert L.nslam_frustum_rows(*a) == -1
    a = list(args)
    a[13] = need - 1                    # short workspace
    assert L.nslam_frustum_rows(*a) == -3


def test_v21_loss_sum_best_validates_without_gpu(pkg):
    """nslam_loss_sum_best needs an output scalar (and a loss vector when there are rays); with a
    best_loss it needs the two camera vectors and 1 <= n <= 64 — all before any launch."""
    L = pkg._lib.lib()
    assert L.nslam_loss_sum_best(4096, 10, None, None, None, None, 0, None) == -1      # no output
    assert L.nslam_loss_sum_best(None, 10, 4096, None, None, None, 0, None) == -1      # no losses
    assert L.nslam_loss_sum_best(4096, -1, 4096, None, None, None, 0, None) == -1      # negative count
    assert L.nslam_loss_sum_best(4096, 10, 4096, 4096, None, 4096, 7, None) == -1     # best without cam
    assert L.nslam_loss_sum_best(4096, 10, 4096, 4096, 4096, 4096, 65, None) == -1    # n > 64


def test_v22_cam_vector_batch_validates_without_gpu(pkg):
    """nslam_cam_vector_batch needs poses and outputs, 1 <= n <= 64 and a pose stride of at least 12 floats
    — all checked before any launch (the copy is optional)."""
    L = pkg._lib.lib()
    assert L.nslam_cam_vector_batch(None, 16, 1, 4096, None, None) == -1     # no poses
    assert L.nslam_cam_vector_batch(4096, 16, 1, None, 4096, None) == -1     # no output
    assert L.nslam_cam_vector_batch(4096, 16, 0, 4096, None, None) == -1     # no cameras
    assert L.nslam_cam_vector_batch(4096, 16, 65, 4096, None, None) == -1    # n > 64
    assert L.nslam_cam_vector_batch(4096, 8, 2, 4096, None, None) == -1      # stride < 12


def test_v23_cam_grad_step_validates_without_gpu(pkg):
    """nslam_cam_grad_step needs its tail (camera, Adam state, step count, loss output; a loss vector when there
    are rays; the best pose with a best loss) before the gradient's own checks — all before any launch."""
    import ctypes
    L = pkg._lib.lib()
    T = pkg._lib.NslamCamTail
    bufs = (ctypes.c_void_p * 1)(4096)

    def call(tail):
        return L.nslam_cam_grad_step(None if tail is None else ctypes.byref(tail), 4096, bufs, 1, 4096, 4096, 10, 4,
                                     4096, 4096, 4096, None)

    def tail(**kw):
        f = dict(cam=4096, exp_avg=4096, exp_avg_sq=4096, step=4096, lr=0.001, beta1=0.9, beta2=0.999, eps=1e-8,
                 ray_loss=4096, n_rays=10, loss_out=4096, best_loss=None, best=None)
        f.update(kw)
        return T(**f)

    assert call(None) == -1
    assert call(tail(cam=None)) == -1
    assert call(tail(step=None)) == -1
    assert call(tail(loss_out=None)) == -1
    assert call(tail(ray_loss=None)) == -1
    assert call(tail(n_rays=-1)) == -1
    assert call(tail(best_loss=4096)) == -1            # best loss without the best pose
    assert L.nslam_cam_grad_step(ctypes.byref(tail()), None, bufs, 1, 4096, 4096, 10, 4, 4096, 4096, 4096,
                                 None) == -1           # the gradient's own checks (no pose)


def test_median_launch_knob_rejects_unknown_values(pkg, monkeypatch):
    """NSLAM_MEDIAN_LAUNCH accepts "0" and "1" only: any other value is NSLAM_EINVAL before any launch."""
    import ctypes
    L = pkg._lib.lib()
    cfg = pkg._lib.NslamLossCfg(pkg._lib.LOSS_TRACKER, 1, 1, 0.5)
    monkeypatch.setenv("NSLAM_MEDIAN_LAUNCH", "yes")
    assert L.nslam_render_loss(ctypes.byref(cfg), 4096, 4096, 4, 48, 4096, 4096, None, 4096, 4096, 4096, 4096,
                               4096, 4096, 5 * 8, None) == -1


def test_v21_gather_frame_needs_a_pose_or_a_camera(pkg):
    """A frame with neither c2w nor cam (ABI v21) is rejected before any launch."""
    L = pkg._lib.lib()
    fr = (pkg._lib.NslamFrame * 1)()
    fr[0].depth, fr[0].color = 4096, 4096
    args = [fr, 1, 10, 4096, 96, 128, 0, 96, 0, 128, 500.0, 500.0, 64.0, 48.0, None, None, 4096, 4096, 4096, 4096,
            None, None, None, None]
    assert L.nslam_gather_rays(*args) == -1


_POINT_EPS = ("fwd", "fwd_ws", "bwd", "bwd_decoder", "bwd_decoders", "bwd_decoders_live", "live_points",
              "color_wgrad")


def _point_call(pkg, ep, pts, n, buf, rays=0, **cfg_fields):
    """One of the eight point-taking entry points on a colour-stage config whose other arguments are all
    acceptable (fake aligned pointers): pts, n and buf (the output row buffer of the forwards, the cotangent
    g_raw of the backwards; nslam_live_points has neither) decide the return code.  rays > 0: the ray form
    with that many samples per ray."""
    lib, L = pkg._lib, pkg._lib.lib()
    cfg = _colour_cfg(pkg)
    cfg.saved_masks = 4096
    if ep == "color_wgrad":
        cfg.act_tape = 4096
        cfg.dgrad[lib.DEC_COLOR].base = 4096
        cfg.dgrad[lib.DEC_COLOR].count = 15575
    if rays:
        cfg.rays_o = cfg.rays_d = cfg.z_vals = 4096
        cfg.n_samples = rays
    for k, v in cfg_fields.items():
        if k == "dgrad_base":
            cfg.dgrad[lib.DEC_COLOR].base = v
        else:
            setattr(cfg, k, v)
    c = ctypes.byref(cfg)
    four = (ctypes.c_void_p * 4)(4096, 4096, 4096, 4096)
    colour, big = 1 << lib.DEC_COLOR, 1 << 62
    if ep == "fwd":
        return L.nslam_query_fwd(c, pts, n, buf, None)
    if ep == "fwd_ws":
        return L.nslam_query_fwd_ws(c, pts, n, buf, 4096, L.nslam_query_fwd_workspace_size(c, n), None)
    if ep == "bwd":
        return L.nslam_query_bwd(c, pts, n, buf, 4096, 4096, big, None)
    if ep == "bwd_decoder":
        return L.nslam_query_bwd_decoder(c, lib.DEC_COLOR, 0, pts, n, buf, 4096, 4096, big, None)
    if ep == "bwd_decoders":
        return L.nslam_query_bwd_decoders(c, colour, pts, n, buf, four, None)
    if ep == "bwd_decoders_live":
        return L.nslam_query_bwd_decoders_live(c, colour, pts, n, buf, four, four, None)
    if ep == "live_points":
        return L.nslam_live_points(c, colour, pts, n, four, four, 4096, big, None)
    assert ep == "color_wgrad"
    return L.nslam_color_wgrad(c, pts, n, buf, 4096, big, None)


# (case, pts, n_pts, buf, samples per ray, config fields): what is wrong with the points of the call
_POINT_CASES = [
    ("negative count", 4096, -1, 4096, 0, {}),
    ("no points", None, 64, 4096, 0, {}),
    ("rays: ragged count", None, 100, 4096, 48, {}),
    ("rays: 2^31 points", None, 1 << 31, 4096, 32, {}),
    ("rays: 2^31 points, ragged", None, (1 << 31) + 1, 4096, 32, {}),
    ("no row buffer", 4096, 64, None, 0, {}),
    # doubly wrong calls: the order of the checks decides the code
    ("negative count, no decoder gradient", 4096, -1, 4096, 0, {"dgrad_base": None}),
    ("no points, no saved masks", None, 64, 4096, 0, {"saved_masks": None}),
    ("no points, parameter gradients asked", None, 64, 4096, 0, {"dgrad_base": 4096}),
    ("no points, d/dpts asked", None, 64, 4096, 0, {"need_pts_grad": 1}),
    ("rays: ragged count, d/dpts asked", None, 100, 4096, 48, {"need_pts_grad": 1}),
    ("no row buffer, parameter gradients asked", 4096, 64, None, 0, {"dgrad_base": 4096}),
    ("no row buffer, no saved masks", 4096, 64, None, 0, {"saved_masks": None}),
]
# pts form: only the live-point entry points index points in 32 bits whatever the form
_LIVE_CASES = [("pts: 2^31 points", 4096, 1 << 31, 4096, 0, {})]

# return codes of the parent commit's library (recorded from its build, before check_points existed), in
# _POINT_EPS order; None: the entry point has no such argument
_POINT_RC = {
    "negative count": (-1, -1, -1, -1, -1, -1, -1, -1),
    "no points": (-1, -1, -1, -1, -1, -1, -1, -1),
    "rays: ragged count": (-1, -1, -1, -1, -1, -1, -1, -1),
    "rays: 2^31 points": (-1, -1, -1, -1, -1, -1, -1, -1),
    "rays: 2^31 points, ragged": (-1, -1, -1, -1, -1, -1, -1, -1),
    "no row buffer": (-1, -1, -1, -1, -1, -1, None, -1),
    "negative count, no decoder gradient": (-1, -1, -1, -1, -1, -1, -1, -1),
    "no points, no saved masks": (-1, -1, -1, -1, -1, -1, -1, -2),
    "no points, parameter gradients asked": (-1, -1, -1, -1, -1, -1, -1, -1),
    "no points, d/dpts asked": (-1, -1, -1, -1, -1, -1, -1, -1),
    "rays: ragged count, d/dpts asked": (-1, -1, -1, -1, -1, -1, -1, -1),
    "no row buffer, parameter gradients asked": (-1, -1, -1, -1, -1, -1, None, -1),
    "no row buffer, no saved masks": (-1, -1, -1, -1, -1, -1, None, -2),
    "pts: 2^31 points": (-1, -1),
}


def test_point_argument_return_codes(pkg):
    """The point-argument checks of the eight point-taking entry points (one check_points helper): every
    entry point returns the code it returned before the checks were merged, for every bad-argument case
    — each before any HIP call."""
    for case, pts, n, buf, rays, fields in _POINT_CASES + _LIVE_CASES:
        want = _POINT_RC[case]
        eps = _POINT_EPS if (case, pts, n, buf, rays, fields) in _POINT_CASES else ("bwd_decoders_live", "live_points")
        assert len(want) == len(eps)
        for ep, rc in zip(eps, want):
            if rc is None:
                continue
            assert rc in (-1, -2, -3), (case, ep)  # an argument error, never a launch
            assert _point_call(pkg, ep, pts, n, buf, rays, **fields) == rc, (case, ep)


_FWD_MODE_CHILD = """
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
cfg = ctypes.create_string_buffer(bytes.fromhex(sys.argv[2]))
vp, i64, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_size_t
L.nslam_query_fwd_workspace_size.argtypes, L.nslam_query_fwd_workspace_size.restype = [vp, i64], sz
L.nslam_query_fwd_ws.argtypes = [vp, vp, i64, vp, vp, sz, vp]
need = L.nslam_query_fwd_workspace_size(cfg, 64)
print(need, L.nslam_query_fwd_ws(cfg, 4096, 64, 4096, 4096, need - int(sys.argv[3]), None))
"""


def test_fwd_mode_rejects_retired_and_unknown_values(pkg):
    """NSLAM_FWD_MODE accepts units (or unset, or empty): the retired dyn, pc and parts and a misspelt value
    are NSLAM_EINVAL before any launch (the variable is read once per process, hence the child processes),
    and the forward workspace keeps its size (the retired variants' 256 reserved bytes included).  The mode
    is checked before the workspace, so an accepted mode shows without a launch: a call one byte short of
    workspace returns NSLAM_EWORKSPACE where a rejected mode returns NSLAM_EINVAL."""
    import sys
    cfg = _colour_cfg(pkg)
    assert pkg._lib.lib().nslam_query_fwd_workspace_size(ctypes.byref(cfg), 64) == 256 + 256
    argv = [sys.executable, "-c", _FWD_MODE_CHILD, pkg._lib.LIB_PATH, bytes(cfg).hex()]
    unset = {k: v for k, v in os.environ.items() if k != "NSLAM_FWD_MODE"}
    # (environment, bytes short of workspace, return code)
    cases = [(dict(unset, NSLAM_FWD_MODE=mode), 0, "-1") for mode in ("dyn", "unit", "pc", "parts")]
    cases += [(dict(unset, NSLAM_FWD_MODE="pc"), 1, "-1"), (dict(unset, NSLAM_FWD_MODE="units"), 1, "-3"),
              (dict(unset, NSLAM_FWD_MODE=""), 1, "-3"), (unset, 1, "-3")]
    kids = [subprocess.Popen(argv + [str(short)], env=env, stdout=subprocess.PIPE, text=True)
            for env, short, _ in cases]
    for kid, (env, short, rc) in zip(kids, cases):
        out = kid.communicate()[0].split()
        assert kid.returncode == 0 and out == ["512", rc], (env.get("NSLAM_FWD_MODE"), short, out)


def test_fwd_variant_rejects_retired_and_unknown_values(pkg):
    """nslam_query_cfg.fwd_variant: 0 (default) and 1 (units) name the one kernel; the retired 2 (pc) and 3
    (parts) and any other value are NSLAM_EINVAL before any launch, with every other argument valid.  An
    accepted value, one byte short of workspace, is NSLAM_EWORKSPACE (no launch either)."""
    L = pkg._lib.lib()
    cfg = _colour_cfg(pkg)
    need = L.nslam_query_fwd_workspace_size(ctypes.byref(cfg), 64)
    for v in (2, 3, -1):
        cfg.fwd_variant = v
        assert L.nslam_query_fwd_workspace_size(ctypes.byref(cfg), 64) == need
        assert L.nslam_query_fwd_ws(ctypes.byref(cfg), 4096, 64, 4096, 4096, need, None) == -1, v
    for v in (0, 1):
        cfg.fwd_variant = v
        assert L.nslam_query_fwd_ws(ctypes.byref(cfg), 4096, 64, 4096, 4096, need - 1, None) == -3, v
