"""TEST INFRASTRUCTURE ONLY: the recipe that compiles the reference's HLSL text for the CPU.

build_ref(reference_dir) reads <reference>/shaders/**/*.hlsl, applies the fixed list of syntax-level rewrites below (HLSL spellings
C++ has no equivalent for; no rule carries shader code as its replacement), writes the result under oracle/_ref/gen/ and compiles
oracle/ref_hlsl_driver.cpp against it and oracle/hlsl_cpu.hpp into

    oracle/_ref/libref_hlsl.so        -fsingle-precision-constant: an unsuffixed literal is a float, as in HLSL
    oracle/_ref/libref_hlsl_wide.so   the same text without that flag: unsuffixed literals are doubles, so the scalar
                                      expressions around them round differently — the reference's own rounding noise

Nothing under oracle/_ref/ is ever committed (.gitignore); tests that need the libraries skip where neither they nor the
reference tree exist.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(_HERE, "_ref")
GEN = os.path.join(OUT, "gen")
DEFAULT_REFERENCE = "/root/reference"

# (pattern, replacement): HLSL syntax -> C++ syntax
REWRITES = [
    (r"\[\[vk::constant_id\(\d+\)\]\]\s*const\s+", "static "),                      # specialization constants become settable variables
    (r"\[\[vk::push_constant\]\]\s*", "static thread_local "),                       # push constants belong to the launch: one set per thread here
    (r"\[\[vk::[^\]]*\]\]\s*", ""),                                                 # binding attributes
    (r"(?m)^[ \t]*\[(?:shader|numthreads)\([^\]]*\)\][ \t]*$", ""),                 # entry-point attributes on their own line
    (r"\[raypayload\]\s*", ""),
    (r"(?:\s*:\s*(?:read|write)\([^)]*\))+", ""),                                   # payload access qualifiers
    (r"\s*:\s*SV_\w+", ""),                                                         # system-value semantics
    (r"\binterface\b", "struct"),
    (r"\b(?:in)?out\s+([\w:]+(?:<[^<>]*>)?)\s+(\w+)", r"\1 &\2"),                   # out / inout parameters are references
    (r"([(,]\s*)in\s+(?=\w)", r"\1"),                                               # `in` parameters are plain
    (r"\breturn\s+this\s*;", "return *this;"),
    # the function that writes the output image first offers its argument to the driver (on_store_color: false = go on as written)
    (r"(\bvoid\s+storeColor\s*\(\s*float3\s+(\w+)\s*\)\s*\{)", r"\1 if (on_store_color(\2)) return;"),
    (r"\bTexture2D\s+(\w+)\s*\[\s*\]\s*;", r"static Texture2D<> *\1;"),             # unsized resource array
    (r"\?\s*(\w+)\s*:\s*(float3\()", r"? float3(\1) : \2"),                         # a ternary mixing uint3 and float3: HLSL's common type
    # C++ leaves the evaluation order of call arguments unspecified; the project assumes DXC's is left to right.  A constructor whose
    # arguments are all draws from a generator becomes a braced initialisation, which C++ orders left to right.
    (r"\b(\w+)\((\s*\w+\.getFloat\(\)(?:\s*,\s*\w+\.getFloat\(\))+\s*)\)", r"\1{\2}"),
]

UNITS = ["main", "equirect", "luminance", "fold"]
COMMON_FLAGS = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-Wall", "-Wextra", "-Wno-comment"]


def _split_top_level(s):
    """the top-level comma-separated parts of an argument list"""
    parts, depth, start = [], 0, 0
    for i, ch in enumerate(s):
        if ch in "({[":
            depth += 1
        elif ch in ")}]":
            depth -= 1
        elif ch == "," and depth == 0:
            parts.append(s[start:i]); start = i + 1
    parts.append(s[start:])
    return parts


def sequence_draws(text):
    """A call two or more of whose arguments draw from a generator (main.hlsl:88) has no evaluation order in C++.  Each such argument is hoisted, left to right, into
    a temporary declared just before the statement; the call then takes the temporaries.  Works on one-line statements, which is how the reference writes them."""
    out, counter = [], 0
    for line in text.split("\n"):
        if line.count(".getFloat()") >= 2 and line.rstrip().endswith(";"):
            for m in re.finditer(r"[\w.]+\(", line):
                if re.match(r"(if|for|while|switch)\(", m.group(0)):
                    continue
                depth, end = 0, None
                for i in range(m.end() - 1, len(line)):
                    depth += line[i] in "({["; depth -= line[i] in ")}]"
                    if depth == 0:
                        end = i; break
                if end is None:
                    continue
                args = _split_top_level(line[m.end():end])
                drawing = [k for k, a in enumerate(args) if ".getFloat()" in a]
                if len(drawing) < 2:
                    continue
                indent = re.match(r"\s*", line).group(0)
                for k in drawing:
                    name = "_seq%d" % counter; counter += 1
                    out.append("%sauto %s = %s;" % (indent, name, args[k].strip()))
                    args[k] = " " + name
                line = line[:m.end()] + ",".join(args) + line[end:]
                break
        out.append(line)
    return "\n".join(out)


def translate(text):
    for pat, rep in REWRITES:
        text = re.sub(pat, rep, text)
    text = sequence_draws(text)
    text = re.sub(r'(#include\s+"[^"]+\.hlsl)"', r'\1.h"', text)
    head = "#pragma GCC system_header\n" + ("" if "#pragma once" in text else "#pragma once\n")
    return head + text + "\n"


def generate(reference_dir):
    src = os.path.join(reference_dir, "shaders")
    written = []
    for base, _, files in os.walk(src):
        for f in sorted(files):
            if not f.endswith(".hlsl"):
                continue
            rel = os.path.relpath(os.path.join(base, f), src)
            dst = os.path.join(GEN, rel + ".h")
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            with open(os.path.join(base, f), encoding="utf-8") as fh:
                out = translate(fh.read())
            with open(dst, "w", encoding="utf-8") as fh:
                fh.write(out)
            written.append(dst)
    return written


def reference_dir():
    return os.environ.get("MSNE_REFERENCE_DIR", DEFAULT_REFERENCE)


def available(ref=None):
    return os.access(os.path.join(ref or reference_dir(), "shaders", "hrtsystem", "main.hlsl"), os.R_OK)      # there and readable


def lib_paths():
    return os.path.join(OUT, "libref_hlsl.so"), os.path.join(OUT, "libref_hlsl_wide.so")


def build_ref(ref=None, cxx="g++"):
    """-> (narrow library, wide library).  Raises if the reference tree is absent."""
    ref = ref or reference_dir()
    if not available(ref):
        raise FileNotFoundError("no reference shaders under %s" % ref)
    generate(ref)
    driver = os.path.join(_HERE, "ref_hlsl_driver.cpp")
    libs = lib_paths()
    for so, extra in zip(libs, (["-fsingle-precision-constant"], [])):
        cmd = [cxx] + COMMON_FLAGS + extra + ["-I", _HERE, "-I", GEN, "-shared", "-o", so + ".tmp"]
        objs = []
        for i, u in enumerate(UNITS):
            o = os.path.join(OUT, "%s_%s.o" % (os.path.basename(so)[:-3], u))
            subprocess.check_call([cxx] + COMMON_FLAGS + extra + ["-I", _HERE, "-I", GEN, "-DREF_UNIT=%d" % i, "-c", driver, "-o", o])
            objs.append(o)
        subprocess.check_call(cmd + objs)
        os.replace(so + ".tmp", so)
        for o in objs:
            os.remove(o)
    return libs


# ----------------------------------------------------------------------------------------------------------------------
# binding
class RefEnv(C.Structure):
    _fields_ = [("rgb", C.c_void_p), ("lum", C.POINTER(C.c_void_p)), ("size", C.c_uint32), ("levels", C.c_uint32)]


def load(path):
    L = C.CDLL(path)
    vp, u32 = C.c_void_p, C.c_uint32
    L.RefProbeBatch.restype = C.c_int; L.RefProbeBatch.argtypes = [C.c_int, vp, u32, vp, C.POINTER(RefEnv)]
    L.RefRngFloats.restype = None; L.RefRngFloats.argtypes = [u32, u32, u32, vp, u32, vp]
    L.RefEnvBuild.restype = C.c_int; L.RefEnvBuild.argtypes = [vp, u32, u32, u32, vp, C.POINTER(vp)]
    L.RefStoreColor.restype = None; L.RefStoreColor.argtypes = [vp, u32, u32, u32, u32, vp]
    L.RefPaths.restype = C.c_int; L.RefPaths.argtypes = [vp, vp, vp, u32, u32, vp, u32, vp, vp, vp, u32, C.c_int]
    return L


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.reshape(shape) if shape is not None else a


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Ref:
    """one of the two libraries, with the same calling surface as oracle.orc where they overlap"""

    def __init__(self, path):
        self.L = load(path)
        self._env = None

    def set_env(self, rgb, lum):
        """the equal-area rgb (S, S, 4) and the luminance pyramid [(S, S), (S/2, S/2), ..., (1, 1)] the env_* probes read"""
        rgb = _f32(rgb); lum = [_f32(l) for l in lum]
        arr = (C.c_void_p * len(lum))(*[l.ctypes.data for l in lum])
        self._env = (RefEnv(rgb.ctypes.data, arr, rgb.shape[0], len(lum)), rgb, lum, arr)

    def probe(self, name, x):
        from oracle.orc import PROBES
        fn, wi, wo = PROBES[name]
        x = _f32(x, (-1, wi)); out = np.zeros((len(x), wo), np.float32)
        env = C.byref(self._env[0]) if self._env is not None else None
        if self.L.RefProbeBatch(fn, _ptr(x), len(x), _ptr(out), env) != 0:
            raise RuntimeError("RefProbeBatch(%s) failed" % name)
        return out

    def rng_floats(self, s, x, y, n):
        out = np.zeros(n, np.float32); st = C.c_uint32()
        self.L.RefRngFloats(s, x, y, _ptr(out), n, C.byref(st))
        return st.value, out

    def env_build(self, rgba, width, height):
        """the three background kernels over their dispatches -> (rgb (S, S, 4), [luminance levels]); S as BackgroundManager.zig:132,154 chooses it"""
        src = _f32(rgba, (height, width, 4))
        S = 1
        while S * 2 <= height:
            S *= 2
        S = min(S, 1024)
        rgb = np.zeros((S, S, 4), np.float32)
        lum = []
        d = S
        while True:
            lum.append(np.zeros((d, d), np.float32))
            if d == 1:
                break
            d //= 2
        arr = (C.c_void_p * len(lum))(*[l.ctypes.data for l in lum])
        if self.L.RefEnvBuild(_ptr(src), width, height, S, _ptr(rgb), arr) != 0:
            raise RuntimeError("RefEnvBuild failed")
        return rgb, lum

    def paths(self, orc_ctx, sensor, lens, jobs, cap=16, threads=8):
        """jobs (n, 3) of (x, y, sample index) on an oracle context -> (radiance (n, 3), hit triples (n, cap, 3), hits per path (n,)):
        the reference's raygen body and integrator, its rays traced by the oracle's search"""
        jobs = np.ascontiguousarray(jobs, dtype=np.uint32).reshape(-1, 3)
        n = len(jobs)
        rgb = np.zeros((n, 3), np.float32); hits = np.full((n, cap, 3), 0xFFFFFFFF, np.uint32); nh = np.zeros(n, np.uint32)
        orc_ctx.L.OrcAliasCount(orc_ctx.h)              # builds the acceleration structure, the inverse transforms and the alias table
        fn = lambda f: C.cast(f, C.c_void_p)
        if self.L.RefPaths(orc_ctx.h, fn(orc_ctx.L.OrcTraceClosest), fn(orc_ctx.L.OrcTraceShadow), sensor, lens, _ptr(jobs), n, _ptr(rgb), _ptr(hits), _ptr(nh), cap, threads) != 0:
            raise RuntimeError("RefPaths failed")
        return rgb, hits, nh

    def store_color(self, film, sample_count, samples_per_run, colors):
        """storeColor (main.hlsl:43-51) of one launch over a whole (h, w, 4) film, in place; colors (h, w, 3) are the launch's summed samples"""
        h, w = film.shape[:2]
        colors = _f32(colors, (h, w, 3))
        assert film.dtype == np.float32 and film.flags.c_contiguous
        self.L.RefStoreColor(_ptr(film), w, h, sample_count, samples_per_run, _ptr(colors))


if __name__ == "__main__":
    print("\n".join(build_ref()))
