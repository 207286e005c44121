#!/usr/bin/env python3
"""One SHA-256 per (module, case, variant, key) of what the path yardsticks under tests/ give, through their public functions alone:
equal output before and after a change to tests/*_ref.py = the yardsticks give the same bytes (dtype and shape are hashed too).
Usage: python tools/yardstick_digest.py > profiles/yardstick_digests.txt      (CPU only; builds the oracle on demand; minutes)"""
import hashlib, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                             # noqa: E402
from oracle import pyoracle as oracle          # noqa: E402
import fresnel_ref as fr                       # noqa: E402
import refract_ref as rf                       # noqa: E402
import render_paths_ref as rpr                 # noqa: E402
import shade_path_ref as sp                    # noqa: E402
import shadow_rule_ref as sh                   # noqa: E402
import visibility_ref as vr                    # noqa: E402

RULES = {"None": None, "SELF": sh.SELF, "NO_SHADOWS": sh.NO_SHADOWS, "ENDED": sh.ENDED}
FRAME = "cubes4_a40"
SHARE = dict(block_rows=8, block_cols=8, block_first=1, block_stride=2)


def emit(module, case, variant, ref):
    for key in sorted(ref):
        a = np.ascontiguousarray(ref[key])
        print(f"{module:16s} {case:14s} {variant:34s} {key:16s} {hashlib.sha256(f'{a.dtype}{a.shape}'.encode() + a.tobytes()).hexdigest()}", flush=True)


def rows():
    for name in sp.FRAMES:
        emit("shade_path_ref", name, "frame_reference", sp.frame_reference(oracle, name))
    for name in sh.LAMPS:
        for label, rule in RULES.items():
            emit("shadow_rule_ref", name, f"rule {label}", sh.case_reference(oracle, name, rule))
    for name in vr.HIDE:
        for which in (0, 1):
            for label in ("None", "SELF"):
                emit("visibility_ref", name, f"triple {which}, rule {label}", vr.case_reference(oracle, name, which, RULES[label]))
    for mod, m in (("refract_ref", rf), ("fresnel_ref", fr)):
        for name in m.DEPTHS:
            for label in ("None", "SELF"):
                emit(mod, name, f"rule {label}", m.case_reference(oracle, name, RULES[label]))


def frames():
    flat, _, lights, refl = sp.frame_case(FRAME)
    lamp = sh.lamp_case(FRAME)[2]
    ior, f0, vis, table = rf.case_ior(flat), fr.case_f0(flat), vr.case_vis(FRAME, 0), vr.case_table(flat)
    t_min = sp.BOUNCE_T_MIN
    calls = {"render_paths_ref": (lights, lambda p, fill: rpr.render_paths(oracle, flat, p, rpr.DEPTH, refl, t_min, fill=fill)),
             "shadow_rule_ref": (lamp, lambda p, fill: sh.render_paths(oracle, flat, p, rpr.DEPTH, refl, t_min, rule=sh.SELF, fill=fill)),
             "visibility_ref": (lamp, lambda p, fill: vr.render_paths(oracle, flat, p, rpr.DEPTH, vis, table, refl, t_min, rule=sh.ENDED, fill=fill)),
             "refract_ref": (lights, lambda p, fill: rf.render_paths(oracle, flat, p, rpr.DEPTH, ior, refl, t_min, rule=sh.SELF, fill=fill)),
             "fresnel_ref": (lights, lambda p, fill: fr.render_paths(oracle, flat, p, rpr.DEPTH, ior, f0, refl, t_min, rule=sh.SELF, fill=fill))}
    for mod, (lit, render) in calls.items():
        for spp in (1, 4):
            for share, kw in (("whole frame", {}), ("tile share", SHARE)):
                for fill in (None, 7):
                    emit(mod, FRAME, f"render_paths spp {spp}, {share}, fill {fill}", render(rpr.camera_params(FRAME, lit, spp=spp, **kw), fill))


if __name__ == "__main__":
    oracle.oracle_lib()
    rows()
    frames()
