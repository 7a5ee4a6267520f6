"""End-to-end probe of the operator entry point: host frames in, homography dict out (upload over PCIe INCLUDED).
usage: python tools/e2e_probe.py [WxH:resize_width:nframes ...]   (default 1280x720:1280:257 and 1920x1080:400:257)
       python tools/e2e_probe.py --ingest bgr,yuv420 --repeats 3 [--root DIR] [--out FILE] [cases ...]
       python tools/e2e_probe.py --assemble TREE.json --baseline A.json,B.json --table profiles/yuv_ingest_e2e.txt

Without --ingest: gray frames replicated to BGR, one timed run per case (the form of the recorded profiles/*_e2e_probe.json).
With --ingest: decoded 4:2:0 planes with non-constant chroma (synthetic.chroma_for); "yuv420" hands them over through
SyntheticYuvCapture (the plane path), "bgr" hands the BGR frames they convert to through SyntheticCapture.  Every case is
warmed up in every format, then the formats alternate `repeats` times; pairs/s of every run is kept so that the spread
between repeats of one format can be set against the difference between formats.
--root DIR measures the package of ANOTHER checkout (e.g. the parent commit exported with `git archive` and built) with
this probe's frames: the frames always come from this tree's synthetic.py.
--baseline: --out files of such runs (same cases, "bgr"), taken in the same session before / after this tree's; --assemble: the
--out file of this tree's run with --ingest bgr,yuv420 (nothing is measured, no GPU needed); --table writes
pairs/s per case, code and format, the spread between repeats of one format, and the two ratios the spread is to be set
against (this tree's BGR path / the baseline's, planes / BGR)."""
import argparse, importlib.util, inspect, json, os, sys, time
import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("cases", nargs="*", default=["1280x720:1280:257", "1920x1080:400:257"])
ap.add_argument("--ingest", default="", help="comma list of bgr, yuv420")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--root", default=HERE, help="checkout whose evenvizion_amd package is measured")
ap.add_argument("--out", default="", help="also write the JSON result here")
ap.add_argument("--baseline", default="", help="comma list of --out files of runs with --root (the parent commit)")
ap.add_argument("--assemble", default="", help="--out file of this tree's run: only write the table")
ap.add_argument("--table", default="", help="write the comparison table here")
args = ap.parse_args()


def table(tree, baselines):
    L = ["End-to-end stream probe: decoded 4:2:0 planes against BGR frames as the source of get_homography_dict",
         "(tools/e2e_probe.py --ingest bgr,yuv420 --repeats N).  ORB only, host frames in -> dictionary out, staging copy and upload",
         "included; every shape warmed up in every format, then the formats alternate.  'baseline' = the parent commit measured with",
         "the same probe and frames (--root) in the same session, before and after this tree.  'bgr' = the BGR frames the planes",
         "convert to (SyntheticCapture), 'yuv420' = the planes (SyntheticYuvCapture); luma a synthetic stream, block chroma.", "",
         "%-20s %-18s %-30s %9s %8s" % ("case (WxH:resize)", "code : format", "pairs/s of the repeats", "median", "spread")]
    for case in [k for k in tree if k != "root"]:
        rows = [("baseline %d : bgr" % (i + 1), b[case]["bgr"]) for i, b in enumerate(baselines)]
        rows[1:1] = [("this : bgr", tree[case]["bgr"]), ("this : yuv420", tree[case]["yuv420"])]
        for name, r in rows:
            L.append("%-20s %-18s %-30s %9.1f %8.1f" % (case.rsplit(":", 1)[0], name, " ".join("%.1f" % v for v in r["pairs_per_s"]),
                                                      r["median"], r["spread"]))
        tb, ty = tree[case]["bgr"], tree[case]["yuv420"]
        spread = max([tb["spread"], ty["spread"]] + [b[case]["bgr"]["spread"] for b in baselines])
        line = "%-20s largest spread between repeats of one format %.1f pairs/s (%.1f %% of this bgr median); yuv420 / bgr = %.3f" % (
            "", spread, 100 * spread / tb["median"], ty["median"] / tb["median"])
        if baselines:
            allb = [v for b in baselines for v in b[case]["bgr"]["pairs_per_s"]]
            line += "; this bgr / baseline bgr = %.3f (baseline median of %d runs %.1f, range %.1f)" % (
                tb["median"] / float(np.median(allb)), len(allb), float(np.median(allb)), max(allb) - min(allb))
        L += [line, ""]
    return "\n".join(L) + "\n"


def write_table(tree):
    text = table(tree, [json.load(open(f)) for f in args.baseline.split(",") if f])
    print(text)
    with open(args.table, "w") as fh:
        fh.write(text)


if args.assemble:
    write_table(json.load(open(args.assemble)))
    sys.exit(0)
spec = importlib.util.spec_from_file_location("probe_synthetic", os.path.join(HERE, "evenvizion_amd", "synthetic.py"))
S = importlib.util.module_from_spec(spec); spec.loader.exec_module(S)
sys.path.insert(0, os.path.abspath(args.root))
from evenvizion_amd.processing.video_processing import get_homography_dict
has_ingest = "ingest" in inspect.signature(get_homography_dict).parameters
formats = [f for f in args.ingest.split(",") if f]
res = {"root": "this tree" if os.path.abspath(args.root) == HERE else args.root}


def run(cap, rw, fmt):
    kw = {"ingest": fmt} if fmt and has_ingest else {}
    t = time.perf_counter()
    d = get_homography_dict(cap, resize_width=rw, features_type_list=["ORB"], **kw)
    return len(d) - 1, time.perf_counter() - t


for case in args.cases:
    wh, rw, nfr = case.split(":")
    w, h = map(int, wh.split("x")); rw = int(rw); nfr = int(nfr)
    gray, _ = S.make_stream(11, 17, w, h)                       # 17 distinct frames, walked there and back
    idx = [i % 32 if i % 32 <= 16 else 32 - i % 32 for i in range(nfr)]
    if not formats:
        frames = [S.gray_to_bgr(gray[i][None])[0] for i in range(17)]
        seq = [frames[i] for i in idx]
        run(S.SyntheticCapture(seq[:66]), rw, "")                # warm-up (context, first import)
        pairs, dt = run(S.SyntheticCapture(seq), rw, "")
        res[case] = dict(pairs=pairs, seconds=round(dt, 3), pairs_per_s=round(pairs / dt, 1))
        continue
    rng = np.random.default_rng(11)
    planes = [(gray[i],) + S.chroma_for(rng, gray[i]) for i in range(17)]
    bgr = [S.yuv420_to_bgr_host(*p) for p in planes] if "bgr" in formats else None
    make = {"bgr": lambda k: S.SyntheticCapture([bgr[i] for i in idx[:k]]),
            "yuv420": lambda k: S.SyntheticYuvCapture([planes[i] for i in idx[:k]])}
    for f in formats:
        run(make[f](66), rw, f)                                  # warm-up of this shape in this format
    rates = {f: [] for f in formats}
    for _ in range(args.repeats):
        for f in formats:
            pairs, dt = run(make[f](nfr), rw, f)
            rates[f].append(round(pairs / dt, 1))
    res[case] = {f: dict(pairs=nfr - 1, pairs_per_s=v, median=float(np.median(v)), spread=round(max(v) - min(v), 1))
                 for f, v in rates.items()}
print(json.dumps(res, indent=1))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)

if args.table:
    write_table(res)
