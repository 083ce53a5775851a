"""The real ModelWrapper step with TWO data-parallel ranks holding different shards, on the one GPU of the box (gloo between
two processes on cuda:0) - round-4 VERDICT "Next round" #2.  The job itself is tests/_two_rank_step.py; tests/conftest.py starts
it before this session initialises the GPU (its ranks must be children of a GPU-clean process) and it runs beside the other
tests.  Contract (/root/reference/main.py:91-94 replaced): after the reducer every rank holds the AVERAGE
of the shards' gradients, so both ranks take the same Adam steps as the CPU oracle fed with averaged gradients."""
import json
import os
import time

import pytest

pytestmark = pytest.mark.gpu


def _record(timeout_s=900.0):
    from conftest import TWO_RANK_JOB
    proc, out = TWO_RANK_JOB["proc"], TWO_RANK_JOB["out"]
    if proc is None:
        pytest.skip("the two-rank job was not started (GPU tests deselected, or no GPU)")
    t0 = time.time()
    while proc.poll() is None and time.time() - t0 < timeout_s:
        time.sleep(1.0)
    assert proc.poll() is not None, "the two-rank job did not finish within %.0f s" % timeout_s
    assert os.path.exists(out), "the two-rank job left no record (exit code %s)" % proc.returncode
    return json.load(open(out))


def test_two_ranks_on_one_gpu_take_the_oracles_averaged_adam_steps():
    rec = _record()
    assert not rec["failures"], "\n".join(rec["failures"][:20]) + "\n--- rank logs ---\n" + "\n".join(rec["logs"])
    assert len(rec["ranks"]) == 2
    for r in rec["ranks"]:
        assert r["ranks_bit_identical"], r
        assert r["native_library"] and r["native_library"].endswith("libsempyr.so"), r     # the HIP path ran in the rank processes
        for mode in ("eager", "graph"):
            m = r[mode]
            assert m["worst_loss_rel_err"] <= 1e-3, (mode, m)
            # a sum instead of an average would show here as 1.0 (Adam itself is blind to a constant gradient scale)
            assert m["grad_norm_rel_err_d"] <= 1e-2 and m["grad_norm_rel_err_g"] <= 1e-2, (mode, m)
            assert m["param_norm_rel_err_d"] <= 1e-3 and m["param_norm_rel_err_g"] <= 1e-3, (mode, m)
    print("two-rank step: " + json.dumps({k: rec["ranks"][0][k] for k in ("eager", "graph")}))


def test_bench_two_rank_dry_run_on_one_gpu():
    """bench.py --gpus 2 with both ranks on this GPU and gloo between them (BENCH_ONE_DEVICE / BENCH_DIST_BACKEND; started by the same
    GPU-clean launcher, after the step job): not a measurement - the first execution of bench.py's N > 1 code path anywhere: it spawns
    its ranks, they rendezvous, agree on the launch mode, run the timed loop with the reducer's collectives, take the max-over-ranks
    clock and rank 0 prints ONE line with the multi-GPU record."""
    rec = _record().get("bench_two_ranks")
    assert rec is not None, "the launcher did not run the bench dry run"
    assert rec["returncode"] == 0 and rec["line"] is not None, rec
    line = rec["line"]
    assert line["n_gpus"] == 2 and line["value"] > 0 and line["scaling"] == "weak" and line["config"]["global_batch"] == 8, line
    mg = line["multi_gpu"]
    assert len(mg["per_rank"]) == 2 and all(v > 0 for v in mg["per_rank"]), mg
    assert rec.get("line_chars", 0) < 4096, rec.get("line_chars")          # the compact line (bench.compact_line), not the full record
    assert mg["allreduce_ms_d"] is not None and mg["allreduce_ms_g"] is not None and mg["grad_bytes_d"] > 0 and mg["grad_bytes_g"] > 0, mg
    assert abs(line["value"] - 8 * line["steps"] / (line["ms_per_step"] * line["steps"] / 1e3)) <= 0.02 * line["value"]
