"""Calibrate the per-lag error budget of the correlation engines (tests/vsg_budget.py), CPU only.

Runs the float32 restatement of the oracle over every case of the lengths table (tests/test_vsg_lengths_gpu.py: all
15 lengths, plus w = 499 and 500), the four flag sets, sub-window multipliers 1, 2, 3 and all six passes, and writes
the worst |err| / (u log2(nfft) beta) per (transform length, flag set) to tests/golden/vsg_budget_calibration.json.
The tests take C = 16 x that ratio.  No kernel is run: the constant never depends on the code under test.

    python tools/measure_vsg_budget.py [--check]     (--check: print, do not write)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import numpy
    import scipy

    from tests import test_vsg_lengths_gpu as lengths
    from tests import vsg_budget as vb
    ratio, at = {}, {}
    for case in vb.lengths_cases():
        for flags, fid in zip(lengths.FLAGS, lengths.FLAG_IDS):
            assert vb.flag_name(flags) == fid
            for mult in vb.MULTS:
                for i in range(lengths.N_PASS):
                    r, unbudgeted = vb.restatement_ratio(case, flags, mult, i)
                    assert unbudgeted == 0, (case, fid, mult, i, unbudgeted)
                    key = (str(case[3]), fid)
                    if r > ratio.get(key, -1.0):
                        ratio[key], at[key] = r, dict(w=case[2], mult=mult, pass_index=i)
    out = dict(
        what="worst |err| / (u log2(nfft) beta) of the float32 restatement of oracle/vsg.py, per transform length and "
             "flag set; the tests' C is 16 x ratio",
        cases=dict(lengths=[list(c) for c in vb.lengths_cases()], flag_sets=lengths.FLAG_IDS, mults=list(vb.MULTS),
                   passes=lengths.N_PASS, n_ch=lengths.N_CH, n_t=lengths.N_T, geometry=lengths.GEO),
        numpy=numpy.__version__, scipy=scipy.__version__, ratio={}, worst_at={})
    for (nfft, fid), r in sorted(ratio.items(), key=lambda kv: (int(kv[0][0]), kv[0][1])):
        out["ratio"].setdefault(nfft, {})[fid] = float(f"{r:.6g}")
        out["worst_at"].setdefault(nfft, {})[fid] = at[(nfft, fid)]
        print(f"nfft {nfft:>4} {fid:<9} ratio {r:.4f}  C {vb.SAFETY * r:.3f}  at {at[(nfft, fid)]}")
    if "--check" not in sys.argv:
        with open(vb.CALIBRATION, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print("wrote", os.path.relpath(vb.CALIBRATION))


if __name__ == "__main__":
    main()
