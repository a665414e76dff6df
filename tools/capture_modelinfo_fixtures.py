"""Capture tests/golden/model_info.npz from the reference's own diameter routine and score tail.

Run by hand where the reference tree exists (ZP_REFERENCE, as tools/capture_bop_fixtures.py reads it):

    python tools/capture_modelinfo_fixtures.py

misc.calc_pts_diameter is imported the way tools/capture_bop_fixtures.py imports misc, and is given
the f64 copy of each f32 cloud, which is what BOP's load_ply hands it.  test.py cannot be imported (its
module top pulls in the whole evaluation stack), so its text is parsed, never stored: the function
compute_auc_posecnn is compiled on its own, and the statements of main() that score one sample
(test.py:465-483) and average the samples (:515-519) are compiled as they stand and run with the pose
error function replaced by one that hands back the stored error.  The file holds data only: the
clouds, the diameters, the error vectors and the numbers the reference made of them.
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from capture_bop_fixtures import REF, import_reference  # noqa: E402
from tests import modelinfo_ref as MR  # noqa: E402
from tests.test_modelinfo_host import CLOUDS, score_cases  # noqa: E402

SAMPLE_LINES, MEAN_LINES = (465, 483), (515, 519)


def _statements(body, first, last):
    """The run of statements spanning exactly lines first .. last, searched through nested bodies."""
    run = [s for s in body if first <= s.lineno and s.end_lineno <= last]
    if run and run[0].lineno == first and run[-1].end_lineno == last:
        return run
    for s in body:
        if s.lineno <= first and last <= s.end_lineno:
            for field in ("body", "orelse", "finalbody"):
                found = _statements(getattr(s, field, []) or [], first, last)
                if found:
                    return found
    return None


def reference_score_tail():
    """-> (compute_auc_posecnn, run(errors, success, diameter) -> dict) made of test.py's own statements."""
    path = os.path.join(REF, "test.py")
    tree = ast.parse(open(path).read(), path)
    fn = next(s for s in tree.body if isinstance(s, ast.FunctionDef) and s.name == "compute_auc_posecnn")
    main = next(s for s in tree.body if isinstance(s, ast.FunctionDef) and s.name == "main")
    ns = {"np": np}
    exec(compile(ast.Module([fn], []), path, "exec"), ns)
    sample = _statements(main.body, *SAMPLE_LINES)
    means = _statements(main.body, *MEAN_LINES)
    assert sample and means, "test.py's score tail is not where the issue's line numbers put it"
    text = ast.unparse(ast.Module(sample + means, []))
    for word in ("adx_error < obj_diameter * 0.1", "ADX_passed_2", "np.linspace(10, 100, num=10)", "sum_correct / 10",
                 "AUC_ADX_error = np.mean(AUC_ADX_error)"):
        assert word in text, word
    sample_code = compile(ast.Module(sample, []), path, "exec")
    means_code = compile(ast.Module(means, []), path, "exec")

    def run(errors, success, diameter):
        N = len(errors)
        env = {"np": np, "obj_diameter": float(diameter), "vertices": None, "r_GT": None, "t_GT": None,
               "R_predict": None, "t_predict": None}
        for name in ("ADX_passed", "ADX_passed_5", "ADX_passed_2", "ADX_error", "AUC_ADX_error"):
            env[name] = np.zeros(N)  # test.py:214-218
        for k in range(N):
            env.update(batch_idx=k, success=bool(success[k]), Calculate_Pose_Error_Main=lambda *a, v=errors[k]: v)
            exec(sample_code, env)
        adx = env["ADX_error"].copy()
        exec(means_code, env)
        return {"pass": np.array([env["ADX_passed"], env["ADX_passed_5"], env["ADX_passed_2"]], np.float64),
                "auc_steps": np.float64(env["AUC_ADX_error"]), "mean_error": np.float64(env["ADX_error_mean"]),
                "auc_posecnn": np.float64(ns["compute_auc_posecnn"](adx / 1000.))}  # test.py:522
    return ns["compute_auc_posecnn"], run


def main():
    misc, _ = import_reference()
    out = {}
    for name, pts in CLOUDS().items():
        assert pts.dtype == np.float32
        out[f"cloud_{name}"] = pts
        out[f"diameter_{name}"] = np.float64(misc.calc_pts_diameter(pts.astype(np.float64)))
        print(name, len(pts), float(out[f"diameter_{name}"]))
    auc, run = reference_score_tail()
    for name, (errors, success, diameter) in score_cases().items():
        got = run(errors, success, diameter)
        out[f"score_{name}_errors"] = errors
        out[f"score_{name}_success"] = success
        out[f"score_{name}_diameter"] = np.float64(diameter)
        for k, v in got.items():
            out[f"score_{name}_{k}"] = v
        print(name, {k: np.round(v, 6) for k, v in got.items()})
    assert MR.dx2_inexact(out["cloud_mixed_257"])
    path = os.path.join(ROOT, "tests", "golden", "model_info.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
