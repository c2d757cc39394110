"""Worker of tests/test_state_parity.py (graph replay vs eager launches): leg A's W40-D20 Single run in a fresh process, so that
the environment it was started with (NNSDP_NO_GRAPH, read once per process) decides how the library launches.
usage: python tests/state_worker.py <iters> <out.json>"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "nn-sdp_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def run(iters: int) -> dict:
    """the digests of raw_multipliers() after `iters` plain iterations and after one check iteration, and the residuals"""
    import hashlib
    import helpers
    import nnsdp_amd as na
    q = helpers.product_query(helpers.load_problem("W40-D20", 0))
    s = na.Solver(q, na.AdmmSdpOptions(decomp_mode=na.SingleDecomp(), max_iters=10 ** 8, proj_tol=1e-12, adapt_every=0, polish=False,
                                       proj_refine=0, minv_mode=1))
    s.iterate(iters)
    res = {"mult_digest": hashlib.sha256(s.raw_multipliers().tobytes()).hexdigest()}
    res["residuals"] = [float(v).hex() for v in s.residuals()]
    res["mult_after_check_digest"] = hashlib.sha256(s.raw_multipliers().tobytes()).hexdigest()
    res["graph_launches"] = s.info(0)
    s.close()
    return res


if __name__ == "__main__":
    with open(sys.argv[2], "w") as fh:
        json.dump(run(int(sys.argv[1])), fh)
