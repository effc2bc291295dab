"""Loader and helpers for the tests against the reference's HLSL text built for the CPU (oracle/ref_hlsl.py).

Loader rule: the libraries under oracle/_ref/ are used if they are there (and not older than the recipe, the header and the driver
where the reference tree is present to rebuild them from); otherwise they are built if the reference tree is there; otherwise the
test skips.  GPU tests read only oracle/_ref/ and liborc.so."""
import os

import numpy as np
import pytest

from moonshine_amd import scenes
from oracle import ref_hlsl

_CACHE = {}


def _stale(libs):
    """older than the recipe, the header, the driver or any header the driver reads the oracle's tables through (a changed layout with old libraries would read wrong memory)"""
    here = os.path.dirname(ref_hlsl.__file__)
    watched = [os.path.join(here, f) for f in ("ref_hlsl.py", "ref_hlsl_driver.cpp", "hlsl_cpu.hpp", "orc_math.h", "orc_scene.h")] + [os.path.join(here, "..", "include", "moonshine_amd.h")]
    newest = max(os.path.getmtime(f) for f in watched)
    return any(os.path.getmtime(p) < newest for p in libs)


def libraries():
    """-> (Ref narrow, Ref wide)"""
    if "libs" not in _CACHE:
        paths = ref_hlsl.lib_paths()
        have = all(os.path.exists(p) for p in paths)
        if ref_hlsl.available() and (not have or _stale(paths)):
            ref_hlsl.build_ref()
        elif not have:
            pytest.skip("neither %s nor the reference tree %s is present" % (paths[0], ref_hlsl.reference_dir()))
        _CACHE["libs"] = (ref_hlsl.Ref(paths[0]), ref_hlsl.Ref(paths[1]))
    return _CACHE["libs"]


class RefProbe:
    """the interface of tests/test_second_source.py's OrcProbe over one of the reference libraries"""

    def __init__(self, ref, env_textures=None):
        self.ref = ref
        if env_textures is None:      # the reference's own preprocessing of the sky
            img = scenes.sky_sun_equirect()
            env_textures = ref.env_build(img, img.shape[1], img.shape[0])
        self.env_textures = env_textures
        ref.set_env(*env_textures)
        self.tex_handles, self.tex_images = [], []

    def __call__(self, name, x):
        return self.ref.probe(name, x)


def noise_tolerance(ref, wide, mag, rel=1e-5, floor=1e-7):
    """8 x the reference's own rounding noise at that input + 1e-5 of the magnitude + 1e-7: the rule of check_values with the two
    builds of the reference's text in the place of the float64 / float32 evaluations of the second source"""
    return 8.0 * np.abs(ref.astype(np.float64) - wide.astype(np.float64)) + rel * mag + floor
