#!/usr/bin/env python3
"""Writes BASELINE.json configs[3] as the reference's driver reads it from disk: a reference directory of FASTA files and an
input directory with one reads file, for sparksmithwaterman_amd.sharded_files (and the control driver).

    python tools/write_config_files.py --config 3 --n-refs 12500 --n-reads 10000 --out DIR [--ref-files 3] [--subdir]

DIR/reference/: synth.config_multi_read's references as ">gi|ref<k>" records of 80-character lines (EngineerData.java:139,
tools/stream_run.py:write_fasta), split over --ref-files files of consecutive references; --subdir puts every second file
into DIR/reference/sub/ so the DirectoryCrawler walk (depth first, sorted) is exercised.  DIR/input/reads1.txt: a leading
">gi" line, then one read per line (InOutOps.GetReads, InOutOps.java:60-88).  Prints one JSON line describing the files.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, choices=(3,), default=3)
    ap.add_argument("--n-refs", type=int, default=12500)
    ap.add_argument("--n-reads", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--ref-files", type=int, default=1)
    ap.add_argument("--subdir", action="store_true")
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)

    from sparksmithwaterman_amd import synth
    from stream_run import write_fasta

    refs, reads = synth.config_multi_read(args.n_refs, args.n_reads, seed=args.seed)
    ref_dir, in_dir = os.path.join(args.out, "reference"), os.path.join(args.out, "input")
    os.makedirs(in_dir, exist_ok=True)
    files = []
    n_files = max(1, min(args.ref_files, len(refs)))
    for f in range(n_files):
        lo, hi = len(refs) * f // n_files, len(refs) * (f + 1) // n_files
        d = os.path.join(ref_dir, "sub") if (args.subdir and f % 2 == 1) else ref_dir
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, "refs%03d.fa" % f)     # (names sort in reference order at each level)
        write_fasta(path, refs[lo:hi], first=lo)
        files.append({"path": path, "refs": hi - lo, "bytes": os.path.getsize(path)})
    reads_path = os.path.join(in_dir, "reads1.txt")
    with open(reads_path, "wb") as f:
        f.write(b">gi|reads configs[3]\n")
        f.write(b"".join(q + b"\n" for q in reads))
    print(json.dumps({"config": args.config, "n_refs": len(refs), "n_reads": len(reads), "ref_dir": ref_dir, "in_dir": in_dir,
                      "ref_files": files, "ref_bases": sum(len(r) for r in refs), "read_bases": sum(len(q) for q in reads)}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
