"""Measures, once and exhaustively, the error of the deterministic math layer (the host build of vr_math.h) against float64 libm, and writes the
maxima with their worst arguments into tests/golden/math_accuracy.json ("exact" section; the "fast" section, measured on a GPU by
tests/test_gpu_math.py's tolerance-mode probe, is kept).  tests/test_math_host.py re-measures on a lattice and holds the result to these figures.

    python tests/tools_math_accuracy.py          # a few minutes on 8 cores: nine unary functions over all 2^32 arguments
    python tests/tools_math_accuracy.py exp_     # only the named functions; the other entries are kept
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hk_math as hm  # noqa: E402

DOMAINS = {hm.LOG: "every positive finite x, denormals included", hm.SIN: "|x| < 8192", hm.COS: "|x| < 8192", hm.TAN: "|x| < 8192",
           hm.SINCOS_S: "|x| < 8192", hm.SINCOS_C: "|x| < 8192", hm.ACOS: "[-1, 1]", hm.ASIN: "[-1, 1]",
           hm.EXP: "[-103.27893, 88.72284], between the cut-offs", hm.NEG_LOG_1M: "every draw k 2^-24, k = 0 .. 2^24 - 1",
           hm.ATAN2: "(z, x) of 2^21 unit directions and the axis-aligned ones", hm.POW: "[0, 1] x 1 / gamma for gamma in [0.25, 8], [0, 1] x sigma in [2^-60, 2^60]"}


def merge(parts):
    best = max(parts, key=lambda p: p["max_ulp"])
    best_abs = max(parts, key=lambda p: p["max_abs"])
    return {"max_ulp": best["max_ulp"], "worst": best["worst"], "max_abs": best_abs["max_abs"], "worst_abs": best_abs["worst_abs"], "points": sum(p["points"] for p in parts)}


def entry(fn, r, exhaustive, domain=None):
    e = {"function": hm.NAMES[fn], "domain": domain or DOMAINS[fn], "exhaustive": exhaustive, "points": r["points"], "max_ulp": r["max_ulp"],
         "worst_bits": ["0x%08x" % r["worst"][0]] + (["0x%08x" % r["worst"][1]] if fn in (hm.ATAN2, hm.POW) else []),
         "worst": [float(hm.f32([w])[0]) for w in r["worst"][:2 if fn in (hm.ATAN2, hm.POW) else 1]]}
    if fn in (hm.SIN, hm.COS, hm.SINCOS_S, hm.SINCOS_C):
        e["max_abs_2p-24"] = r["max_abs"] * 2.0 ** 24
        e["worst_abs_bits"] = "0x%08x" % r["worst_abs"][0]
    return e


def main():
    doc = hm.recorded() if os.path.exists(hm.ACCURACY_JSON) else {}
    only = set(sys.argv[1:])
    out = dict(doc.get("exact") or {}) if only else {}
    for fn in (hm.LOG, hm.SIN, hm.COS, hm.TAN, hm.ACOS, hm.EXP, hm.ASIN, hm.SINCOS_S, hm.SINCOS_C):
        if only and hm.NAMES[fn] not in only:
            continue
        r = merge([hm.accuracy_sweep(fn, k << 28, 1 << 28) for k in range(16)])
        out[hm.NAMES[fn]] = entry(fn, r, True)
        print(out[hm.NAMES[fn]], flush=True)
    for fn in (hm.SINCOS_S, hm.SINCOS_C):          # the angles the renderer forms: far from the large arguments where a zero of the function costs hundreds of ulps
        name = hm.NAMES[fn] + hm.LIVE
        if not only or name in only:
            chunks = [(k, min(1 << 28, hm.TWO_PI_BITS + 1 - k)) for k in range(0, hm.TWO_PI_BITS + 1, 1 << 28)]
            out[name] = entry(fn, merge([hm.accuracy_sweep(fn, k, n) for k, n in chunks]), True, "[0, 2 pi]")
            print(out[name], flush=True)
    for fn, args, exhaustive in ((hm.NEG_LOG_1M, (hm.draws(),), True), (hm.ATAN2, hm.unit_directions(), False), (hm.POW, hm.pow_domains(), False)):
        if not only or hm.NAMES[fn] in only:
            out[hm.NAMES[fn]] = entry(fn, hm.accuracy(fn, *args), exhaustive)
    doc["unit"] = "ulps of the correctly rounded float32 result; max_abs_2p-24 in units of 2^-24; reference: float64 libm"
    doc["exact"] = out
    doc.setdefault("fast", None)
    with open(hm.ACCURACY_JSON, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", hm.ACCURACY_JSON)


if __name__ == "__main__":
    main()
