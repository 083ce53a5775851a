#!/usr/bin/env python3
"""Times the pair-set kernels of csrc/metrics.hip against the same results formed with torch on the same device, in the same job.

    python tools/time_metrics.py [--sizes 6000,50000] [--reps 5] [--ops knn,cover,poly3,is] [--out profiles/metrics_ab.txt]

Synthetic non-negative features (ReLU of normals), d = 2048, N = M per size:
    knn     the radii of one set (k = 5, own row skipped)        torch: fp32 mm per column chunk + topk, merged by a second topk
    cover   counts against both radii and both minima, one pass  torch: fp32 mm per column chunk + comparisons and sums / minima
    poly3   the three Gram sums of KID, 100 subsets x 1 000 rows torch: gathered fp32 bmm + float64 cube and sum
    is      the Inception Score of one set under a 1000-class head (normal rows scaled by 2 / sqrt(d)), 10 splits:
            is_lse (sp_pairset_lse), is_colsum (sp_pairset_softmax_colsum) and is_kl (metrics.inception_kl whole: workspace, both
            passes, the transfer)                                torch: fp32 addmm, then float64 log_softmax and sums (per pass: the
                                                                 logits formed again, as the library forms them)
The two are alternated, after one warm-up run each, and the median of --reps runs is reported, with the library's fraction of the
157.3 TFLOP/s fp32 MFMA peak (2 N M d flop per pass; poly3: 3 x 100 x 2 m^2 d).  One JSON line per (size, entry point); the lines
also go to --out.  Each size runs in a child process under `timeout`, so a stuck step ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32 = 157.3e12
D, K, CHUNK = 2048, 5, 8192
IS_CLASSES, IS_SPLITS = 1000, 10


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _ab(ours, theirs, reps):
    """One warm-up each, then alternate; medians in seconds and the last results."""
    ours(); theirs()
    a, b = [], []
    for _ in range(reps):
        t, ra = _timed(ours)
        a.append(t)
        t, rb = _timed(theirs)
        b.append(t)
    return statistics.median(a), statistics.median(b), ra, rb


def child(n, reps, which):
    import torch
    from semantic_pyramid_for_image_generation_amd import metrics as M
    from semantic_pyramid_for_image_generation_amd import ops
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(n)
    a = torch.relu(torch.randn((n, D), device="cuda", generator=g))
    b = torch.relu(torch.randn((n, D), device="cuda", generator=g))
    lines = []

    def report(name, flop, t_lib, t_torch, agree):
        line = {"n": n, "d": D, "op": name, "lib_ms": round(t_lib * 1e3, 2), "torch_ms": round(t_torch * 1e3, 2),
                "lib_tflops": round(flop / t_lib / 1e12, 1), "lib_frac_of_f32_mfma_peak": round(flop / t_lib / PEAK_F32, 3), "agree": agree}
        lines.append(line)
        print(json.dumps(line), flush=True)

    if "is" in which:
        child_is(n, reps, a, report)
    if not {"knn", "cover", "poly3"} & set(which):
        return lines
    ws = torch.empty((max(ops.pairset_workspace_bytes(n, n, D, K), 8) + 7) // 8, dtype=torch.float64, device="cuda")
    print(json.dumps({"n": n, "workspace_bytes": ops.pairset_workspace_bytes(n, n, D, K)}), flush=True)

    def torch_knn(x):
        nx = (x * x).sum(1)
        best = None
        for c0 in range(0, n, CHUNK):
            y = x[c0:c0 + CHUNK]
            dist = ((nx[:, None] + nx[None, c0:c0 + CHUNK]) - 2.0 * (x @ y.T)).clamp_min_(0)
            idx = torch.arange(c0, min(c0 + CHUNK, n), device=x.device)
            dist[idx, idx - c0] = float("inf")
            top = dist.topk(K, dim=1, largest=False).values
            best = top if best is None else torch.cat([best, top], 1).topk(K, dim=1, largest=False).values
        return best[:, K - 1]

    t_lib, t_torch, r_lib, r_torch = _ab(lambda: ops.pairset_knn(a, a, K, same=True, workspace=ws), lambda: torch_knn(a), reps)
    rel = float(((r_lib - r_torch).abs() / r_torch.clamp_min(1e-30)).max())
    report("knn", 2.0 * n * n * D, t_lib, t_torch, "max rel diff of radii %.2e" % rel)
    rad_a, rad_b = r_lib, ops.pairset_knn(b, b, K, same=True, workspace=ws)

    def torch_cover():
        na, nb = (a * a).sum(1), (b * b).sum(1)
        row_count = torch.zeros(n, dtype=torch.int64, device="cuda")
        row_min = torch.full((n,), float("inf"), device="cuda")
        col_count, col_min = [], []
        for c0 in range(0, n, CHUNK):
            dist = ((na[:, None] + nb[None, c0:c0 + CHUNK]) - 2.0 * (a @ b[c0:c0 + CHUNK].T)).clamp_min_(0)
            row_count += (dist <= rad_b[None, c0:c0 + CHUNK]).sum(1)
            row_min = torch.minimum(row_min, dist.min(1).values)
            col_count.append((dist <= rad_a[:, None]).sum(0))
            col_min.append(dist.min(0).values)
        return row_count, torch.cat(col_count), row_min, torch.cat(col_min)

    t_lib, t_torch, r_lib, r_torch = _ab(lambda: ops.pairset_cover(a, b, rad_a=rad_a, rad_b=rad_b, workspace=ws), torch_cover, reps)
    off = max(int((r_lib[i].long() - r_torch[i]).abs().max()) for i in (0, 1))
    report("cover", 2.0 * n * n * D, t_lib, t_torch, "max count diff %d (fp32 ties), sum %d vs %d"
           % (off, int(r_lib[0].sum()), int(r_torch[0].sum())))

    subsets, m = 100, min(1000, n)
    ix, iy, _ = M.kid_indices(n, n, subsets, m, 0)
    ixd, iyd = torch.from_numpy(ix).cuda(), torch.from_numpy(iy).cuda()
    ws3 = torch.empty((subsets * ops.pairset_workspace_bytes(m, m, D, 0) + 7) // 8, dtype=torch.float64, device="cuda")

    def lib_poly3():
        return torch.stack([ops.pairset_poly3(b, ixd, b, ixd, subsets, m, True, workspace=ws3),
                            ops.pairset_poly3(a, iyd, a, iyd, subsets, m, True, workspace=ws3),
                            ops.pairset_poly3(b, ixd, a, iyd, subsets, m, False, workspace=ws3)])

    def torch_poly3():
        x, y = b[ixd.long()], a[iyd.long()]                       # (subsets, m, D)
        out = []
        for p, q, skip in ((x, x, True), (y, y, True), (x, y, False)):
            k3 = (torch.bmm(p, q.transpose(1, 2)).double() / D + 1.0) ** 3
            s = k3.sum((1, 2))
            out.append(s - torch.diagonal(k3, dim1=1, dim2=2).sum(1) if skip else s)
        return torch.stack(out)

    t_lib, t_torch, r_lib, r_torch = _ab(lib_poly3, torch_poly3, reps)
    rel = float(((r_lib - r_torch).abs() / r_torch.abs()).max())
    report("poly3", 3.0 * subsets * 2.0 * m * m * D, t_lib, t_torch, "max rel diff of sums %.2e" % rel)
    return lines


def child_is(n, reps, a, report):
    """The Inception Score rows: each pass and the whole inception_kl against torch on the same device."""
    import torch
    from semantic_pyramid_for_image_generation_amd import metrics as M
    from semantic_pyramid_for_image_generation_amd import ops
    g = torch.Generator(device="cuda").manual_seed(n + 1)
    w = torch.randn((IS_CLASSES, D), device="cuda", generator=g) * (2.0 / D ** 0.5)
    bias = 0.1 * torch.randn(IS_CLASSES, device="cuda", generator=g)
    need = ops.pairset_softmax_workspace_bytes(n, IS_CLASSES, D, IS_SPLITS)
    print(json.dumps({"n": n, "classes": IS_CLASSES, "splits": IS_SPLITS, "is_workspace_bytes": need,
                      "fp32_logit_matrix_bytes": 4 * n * IS_CLASSES}), flush=True)
    ws = torch.empty((need + 7) // 8, dtype=torch.float64, device="cuda")
    bounds = [(s * n // IS_SPLITS, (s + 1) * n // IS_SPLITS) for s in range(IS_SPLITS)]
    flop = 2.0 * n * IS_CLASSES * D

    def torch_lse():
        l = torch.addmm(bias, a, w.t()).double()
        lp = torch.log_softmax(l, dim=1)
        return l[:, 0] - lp[:, 0], (lp.exp() * lp).sum(1)

    def torch_colsum(lse, h):
        p = (torch.addmm(bias, a, w.t()).double() - lse[:, None]).exp()
        cs = torch.stack([p[lo:hi].sum(0) for lo, hi in bounds])
        q = cs / torch.tensor([hi - lo for lo, hi in bounds], dtype=torch.float64, device="cuda")[:, None]
        hm = torch.stack([h[lo:hi].mean() for lo, hi in bounds])
        return cs, hm - torch.where(q > 0, q * q.log(), torch.zeros_like(q)).sum(1)

    def torch_kl():                                               # the whole score the way torch would form it: the logits ONCE, kept
        lp = torch.log_softmax(torch.addmm(bias, a, w.t()).double(), dim=1)
        p = lp.exp()
        h = (p * lp).sum(1)
        q = torch.stack([p[lo:hi].mean(0) for lo, hi in bounds])
        hm = torch.stack([h[lo:hi].mean() for lo, hi in bounds])
        return (hm - torch.where(q > 0, q * q.log(), torch.zeros_like(q)).sum(1)).cpu().numpy()

    t_lib, t_torch, r_lib, r_torch = _ab(lambda: ops.pairset_lse(a, w, bias, workspace=ws), torch_lse, reps)
    lse, h = r_lib
    diff = max(float((r_lib[i] - r_torch[i]).abs().max()) for i in (0, 1))
    report("is_lse", flop, t_lib, t_torch, "max abs diff of lse / h %.2e" % diff)
    t_lib, t_torch, r_lib, r_torch = _ab(lambda: ops.pairset_softmax_colsum(a, w, bias, lse, h, IS_SPLITS, workspace=ws),
                                         lambda: torch_colsum(lse, h), reps)
    report("is_colsum", flop, t_lib, t_torch, "max abs diff of kl %.2e, of colsum %.2e"
           % (float((r_lib[1] - r_torch[1]).abs().max()), float((r_lib[0] - r_torch[0]).abs().max())))
    t_lib, t_torch, r_lib, r_torch = _ab(lambda: M.inception_kl(a, w, bias, splits=IS_SPLITS), torch_kl, reps)
    score = M.inception_score_from_kl(r_lib)
    report("is_kl", 2.0 * flop, t_lib, t_torch, "max abs diff of kl %.2e; IS %.4f +- %.4f (torch forms the logits once and keeps %d MB of float64)"
           % (float(abs(r_lib - r_torch).max()), score["inception_score"], score["inception_score_std"], 8 * n * IS_CLASSES // 1000000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="6000,50000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ops", default="knn,cover,poly3,is", help="which rows: knn, cover and poly3 run together; is = the Inception Score")
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child is not None:
        child(a.child, a.reps, a.ops.split(","))
        return
    text = []
    for n in a.sizes.split(","):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", n, "--reps", str(a.reps), "--ops", a.ops]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        sys.stdout.write(proc.stdout)
        sys.stdout.flush()
        text.append(proc.stdout)
        if proc.returncode != 0:
            print(json.dumps({"n": int(n), "error": "exit status %d" % proc.returncode}), flush=True)
            sys.exit(1)                 # a failed / stuck GPU step ends the run
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/time_metrics.py --sizes %s --reps %d --ops %s: library vs torch, alternated, medians\n" % (a.sizes, a.reps, a.ops))
            f.write("".join(text))


if __name__ == "__main__":
    main()
