"""usage: bvh_audit_variants.py — soups of 257 and 4097 triangles and the instanced S2 built by the shipped library under the builder route set in the environment
(it is read when a context is made), each audited I1-I5 (tests/bvh_audit.py).  Prints AUDIT_OK."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from moonshine_amd import api
import bvh_audit
from parity_scenes import build_case

for name in ("257", "4097", "s2"):
    rec = bvh_audit.SceneRecorder(api.Context())
    planted = build_case(rec, name)
    bvh_audit.assert_clean(bvh_audit.audit(rec.read_bvh(), rec), planted, name)
print("AUDIT_OK")
