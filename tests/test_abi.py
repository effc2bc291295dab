"""CPU tests: the C-ABI library loads and exports every symbol include/moonshine_amd.h declares; struct layouts match
hydra/moonshine.h.  No compute call is made (there is no GPU here, and there is no CPU fallback)."""
import ctypes as C
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(gpu_api):
    L = gpu_api.load_library()
    hdr = open(os.path.join(ROOT, "include", "moonshine_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b((?:HdMoonshine|Msne)[A-Za-z0-9]+)\s*\(", hdr))
    assert len([d for d in declared if d.startswith("HdMoonshine")]) == 24        # hydra/moonshine.h:72-95
    bound = {s[0] for s in gpu_api.SYMBOLS}
    assert declared == bound, (declared ^ bound)
    for name in declared:
        assert hasattr(L, name), name


# diagnostics (header part 3) a renderer front end never calls: the Zig binding leaves them out
_ZIG_LEAVES_OUT = {"MsneSetProfiling", "MsneGetAccelStats", "MsneGetTexelPoolBytes", "MsneSetBuildQuality", "MsneGetTraversalCounters", "MsneGetTraversalLaneUse",
                   "MsneGetBounceCounters", "MsneGetLaunchTimes", "MsneTraceRays", "MsneShadeProbe", "MsneGetEnvSize", "MsneReadEnv", "MsneGetAliasTable", "MsneReadBvh", "MsneProbeClockGhz"}


def _split_args(a):
    out, depth, cur = [], 0, ""
    for ch in a:
        if ch in "([{": depth += 1
        if ch in ")]}": depth -= 1
        if ch == "," and depth == 0:
            out.append(cur); cur = ""
        else:
            cur += ch
    if cur.strip() and cur.strip() != "void":
        out.append(cur)
    return out


def test_zig_binding_declares_the_headers_entry_points():
    """moonshine_amd/host/zig/amd.zig (the file INTEGRATION.md section 2 hands a maintainer of the reference; no Zig toolchain in this image, so it is NOT compiled here):
    every entry point of parts 1 and 2 of the header is declared `pub extern fn` with the header's number of arguments, and nothing is declared that the header lacks"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "moonshine_amd.h")).read(), flags=re.S)
    c_decl = {m.group(1): len(_split_args(m.group(2))) for m in re.finditer(r"\b((?:HdMoonshine|Msne)[A-Za-z0-9]+)\s*\(([^;{]*)\)\s*;", hdr) if not m.group(1).endswith("Fn")}
    zig = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "moonshine_amd", "host", "zig", "amd.zig")).read())
    z_decl = {m.group(1): len(_split_args(m.group(2))) for m in re.finditer(r"pub extern fn (\w+)\(([^;]*)\)\s*[^;]*;", zig)}
    assert set(z_decl) <= set(c_decl), set(z_decl) - set(c_decl)
    assert set(c_decl) - set(z_decl) == _ZIG_LEAVES_OUT, (set(c_decl) - set(z_decl)) ^ _ZIG_LEAVES_OUT
    for name, n in z_decl.items():
        assert c_decl[name] == n, (name, c_decl[name], n)
    for f in ("offline.zig", "furnace_test.zig"):   # what they call exists in the binding
        src = open(os.path.join(ROOT, "moonshine_amd", "host", "zig", f)).read()
        for name in set(re.findall(r"amd\.((?:HdMoonshine|Msne)\w+)\(", src)):
            assert name in z_decl, (f, name)


def test_struct_layouts_match_reference_header(gpu_api):
    a = gpu_api
    assert C.sizeof(a.F32x2) == 8 and C.sizeof(a.F32x3) == 12 and C.sizeof(a.F32x4) == 16
    assert C.sizeof(a.Mat3x4) == 48                      # moonshine.h:33-35
    assert C.sizeof(a.Geometry) == 12                    # moonshine.h:37-41 (u32, u32, bool + pad)
    assert C.sizeof(a.Lens) == 48                        # moonshine.h:48-55 / Camera.zig:18-25
    assert C.sizeof(a.Material) == 24                    # moonshine.h:57-64
    assert C.sizeof(a.MsnePipelineOpts) == 28            # pipeline.zig:319-327: 7 x 4 B spec constants
    assert C.sizeof(a.Extent2D) == 8


def test_no_cpu_fallback_without_gpu(gpu_api):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(gpu_api.MoonshineError):
        gpu_api.Context()          # must fail loudly, not fall back to a CPU path
    L = gpu_api.load_library()
    assert L.HdMoonshineCreate() in (None, 0)            # hydra.zig:107-143: NULL on init failure
    assert b"HIP device" in L.MsneGetLastError(None)


def test_product_never_imports_the_oracle():
    """the oracle is test infrastructure: nothing under moonshine_amd/ or include/ may import, include, link or load it"""
    pat = re.compile(r"(^\s*(from|import)\s+oracle\b)|(#include\s*[\"<][^\">]*orc_)|(liborc)|(\boracle[./]orc)", re.M)
    for top in ("moonshine_amd", "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".hip", ".h", ".cpp", ".c")):
                    src = open(os.path.join(dirpath, f), errors="ignore").read()
                    assert not pat.search(src), (f, pat.search(src).group(0))


def canonical_decls(text):
    """The declarations of a C header as data: handle typedefs, opaque structs, struct fields, enum members and function signatures (parameter
    names dropped), comments and spacing ignored, sorted.  tests/golden/hydra_abi.json holds the SHA-256 of this form of the reference's
    hydra/moonshine.h."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)

    def norm(t):
        return re.sub(r"\s*\*\s*", "*", " ".join(t.split()))
    out = [["typedef", m.group(1), m.group(2)] for m in re.finditer(r"typedef\s+(\w+)\s+(\w+)\s*;", text)]
    out += [["opaque", m.group(1), m.group(2)] for m in re.finditer(r"typedef\s+struct\s+(\w+)\s+(\w+)\s*;", text)]
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for decl in m.group(2).split(";"):
            if decl.strip():
                ty, names = re.match(r"\s*(.*?)\s+(\w+(?:\s*,\s*\w+)*)\s*$", decl, flags=re.S).groups()
                fields += [[norm(ty), n.strip()] for n in names.split(",")]
        out.append(["struct", m.group(1), m.group(3), fields])
    for m in re.finditer(r"typedef\s+enum\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        out.append(["enum", m.group(1), m.group(3), [e.strip() for e in m.group(2).split(",") if e.strip()]])
    for m in re.finditer(r"(?:extern\s+\"C\"\s+)?([A-Za-z_][\w\s*]*?)\s*\b(HdMoonshine\w+)\s*\(([^;{]*)\)\s*;", text):
        params = []
        for p in m.group(3).split(","):
            toks = norm(p).replace("*", " * ").split()
            if len(toks) >= 2 and re.fullmatch(r"[A-Za-z_]\w*", toks[-1]) and toks[-2] != "const":
                toks = toks[:-1]                  # a parameter name
            t = norm(" ".join(toks))
            if t and t != "void":
                params.append(t)
        out.append(["function", norm(m.group(1)), m.group(2), params])
    return sorted(out, key=json.dumps)


def test_canonical_decls_sees_every_change_of_a_declaration():
    """the canonical form keeps what a caller compiles against: a changed parameter type, field, enum member or return type changes it; comments,
    spacing and parameter names do not"""
    base = '''typedef uint32_t MeshHandle; typedef struct F32x2 { float x, y; } F32x2; typedef enum TextureFormat { f16x4, u8x4_srgb } TextureFormat;
    typedef struct HdMoonshine HdMoonshine; extern "C" MeshHandle HdMoonshineCreateMesh(HdMoonshine*, const F32x2*, size_t);'''
    same = base.replace("const F32x2*, size_t)", "const F32x2 * texcoords /* face-varying */, size_t count)").replace("{ float x, y; }", "{\n    float x,\n    y;\n}")
    assert canonical_decls(same) == canonical_decls(base)
    for a, b in (("size_t)", "uint32_t)"), ("const F32x2*", "F32x2*"), ("float x, y;", "double x, y;"), ("u8x4_srgb }", "u8x4_srgb, f32x4 }"),
                 ("extern \"C\" MeshHandle", "extern \"C\" ImageHandle"), ("float x, y;", "float y, x;")):
        assert canonical_decls(base.replace(a, b)) != canonical_decls(base), (a, b)
    assert len([d for d in canonical_decls(base) if d[0] == "function"]) == 1


def test_translation_unit_built_against_the_reference_header_links_and_loads(tmp_path, gpu_api):
    """drop-in at the link level.  Part 1 of include/moonshine_amd.h declares exactly what the reference's hydra/moonshine.h (the header
    hydra/*.cpp include) declares — its canonical form hashes to the value tests/golden/hydra_abi.json records for the reference header — so a
    C++ file that calls all 24 entry points through those declarations compiles (-Wall -Werror), links against libmoonshine_amd.so and starts
    (nothing is executed: no GPU here)."""
    import hashlib
    import subprocess
    from moonshine_amd import build as b
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "hydra_abi.json")))
    header = os.path.join(ROOT, "include", "moonshine_amd.h")
    hdr = open(header, encoding="utf-8").read()
    part1 = canonical_decls(hdr[hdr.index("Part 1 \u2014"):hdr.index("Part 2 \u2014")])
    assert len(part1) == golden["declarations"] and len([d for d in part1 if d[0] == "function"]) == golden["entry_points"]
    assert hashlib.sha256(json.dumps(part1).encode()).hexdigest() == golden["sha256"], "part 1 of include/moonshine_amd.h no longer declares what hydra/moonshine.h declares"
    src = tmp_path / "hydra_tu.cpp"
    src.write_text('''#include "%s"
int main(int argc, char** argv) {
    if (argc < 1000) return 0;            // never true: the calls below only have to compile and link
    HdMoonshine* c = HdMoonshineCreate();
    F32x3 p[3] = {}; F32x2 t[3] = {}; U32x3 i[1] = {}; uint8_t px[8] = {};
    MeshHandle m = HdMoonshineCreateMesh(c, p, p, t, 3, i, 1);
    ImageHandle i1 = HdMoonshineCreateSolidTexture1(c, 0.5f, "a"), i2 = HdMoonshineCreateSolidTexture2(c, F32x2{0, 0}, "b");
    ImageHandle i3 = HdMoonshineCreateSolidTexture3(c, F32x3{0, 0, 0}, "c"), i4 = HdMoonshineCreateRawTexture(c, px, Extent2D{1, 1}, u8x4_srgb, "d");
    MaterialHandle mat = HdMoonshineCreateMaterial(c, Material{i2, i3, i4, i1, i1, 1.5f});
    HdMoonshineSetMaterialNormal(c, mat, i2); HdMoonshineSetMaterialEmissive(c, mat, i3); HdMoonshineSetMaterialColor(c, mat, i3);
    HdMoonshineSetMaterialMetalness(c, mat, i1); HdMoonshineSetMaterialRoughness(c, mat, i1); HdMoonshineSetMaterialIOR(c, mat, 1.3f);
    Geometry g{m, mat, false};
    Mat3x4 x{};
    InstanceHandle in = HdMoonshineCreateInstance(c, x, &g, 1, true);
    HdMoonshineSetInstanceTransform(c, in, x); HdMoonshineSetInstanceVisibility(c, in, false); HdMoonshineDestroyInstance(c, in);
    SensorHandle s = HdMoonshineCreateSensor(c, Extent2D{4, 4});
    Lens l{};
    LensHandle lh = HdMoonshineCreateLens(c, l); HdMoonshineSetLens(c, lh, l);
    bool ok = HdMoonshineRebuildPipeline(c) && HdMoonshineRender(c, s, lh);
    float* d = HdMoonshineGetSensorData(c, s);
    HdMoonshineDestroy(c);
    return ok && d ? 0 : 1;
}
''' % header)
    exe = tmp_path / "hydra_tu"
    libdir = os.path.dirname(b.LIB)
    # -Wno-comment: the header's comments name paths like hydra/*.cpp (the library itself is built with the same flag)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-comment", "-o", str(exe), str(src), "-L" + libdir, "-lmoonshine_amd", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath-link," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")])
    assert subprocess.run([str(exe)], timeout=120).returncode == 0
