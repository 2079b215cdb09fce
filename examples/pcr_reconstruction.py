"""Principal-component regression on the Nakhon Phanom data (the reference's bundled NPannual / NPpc): the
examples of R/PCR.R -- PCR_reconstruction(NPannual, NPpc, start.year = 1200), cvPCR(NPannual, NPpc,
start.year = 1200) on NPcv's folds, and PCR_ensemble_selection(NPannual, list(NPpc, NPpc[, 1:2]), ...,
agg.type = 'best overall', criterion = 'KGE') -- every least-squares fit on the GPU.
usage: python examples/pcr_reconstruction.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ldsr_amd  # noqa: E402


def main():
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_data.json")))
    Qa = {"year": np.array(ref["NPannual"]["year"]), "Qa": np.array(ref["NPannual"]["Qa"])}
    pc = np.ascontiguousarray(np.array(ref["NPpc"]["data"]).T)             # 813 x 3, years 1200..2012
    Z = [np.array(z) - 1 for z in ref["NPcv"]["Z"]]                        # stored 1-based

    rec = ldsr_amd.PCR_reconstruction(Qa, pc, start_year=1200)
    print("PCR_reconstruction: coefficients %s, sigma %.6f" % (np.array2string(rec["coeffs"], precision=6), rec["sigma"]))
    for i in (0, 400, 812):
        print("  %d: Q %.1f  [%.1f, %.1f]" % (rec["rec"]["year"][i], rec["rec"]["Q"][i], rec["rec"]["Ql"][i], rec["rec"]["Qu"][i]))

    cvr = ldsr_amd.cvPCR(Qa, pc, start_year=1200, Z=Z)
    print("cvPCR, %d folds: %s" % (len(Z), ", ".join("%s %.4f" % kv for kv in cvr["metrics"].items())))

    sel = ldsr_amd.PCR_ensemble_selection(Qa, [pc, pc[:, :2]], start_year=1200, Z=Z, agg_type="best overall",
                                          criterion="KGE", return_all_metrics=True)
    print("PCR_ensemble_selection: choice %d (0 = the ensemble mean), KGE of the members and the ensemble: %s"
          % (sel["choice"], np.array2string(sel["all_metrics"]["KGE"], precision=4)))


if __name__ == "__main__":
    main()
