"""File-to-file driver with every reference file sharded over the ranks (BASELINE.json configs[3] as specified).

Distribution.DistributeReference.call (src/sw/Distribution.java:227-373) walks the reads directory; for every reads file it
maps every reference of every reference file against all reads (:329-338), reduces to the best total(s) and writes
`result<N>.txt` (:355-365, InOutOps.java:244-288).  Here rank r of `world` streams, for each reference file, only its byte-range
shard of the file (swmi_stream_push_file_shard, include/swmi_io.h: swmi_io_read_refs_shard) through the scores-only sweep
(options scores_only = 1, stream_keep_records = 0) and keeps nothing but its candidates -- the references at its running
maximum.  The reduce is the control path's (`int max = 0`, ties kept, Distribution.java:573,600-613) over the ranks, with
(file index, byte offset of the metadata line) as the reference's key, i.e. the order in which NoDistribution meets it.  The
owning rank aligns each winner once more with the full path (sweep, tied maxima, traceback, strings) and sends (key,
metadata, sequence, match sites) to rank 0 over gloo; rank 0 merges them in key order, sorts them stably by metadata
(OptSeqsComp, :647-666) and writes the file.  Totals reduce over RCCL ("nccl") with one rank per GPU, over gloo when ranks
share a GPU (SWMI_ONE_GPU=1).

    python -m sparksmithwaterman_amd.sharded_files --ref-dir R --in-dir I --out-dir O --world N   (starts its own ranks)
"""
import json
import os
import time

import numpy as np

from . import _capi
from . import io as _io
from . import distributed as swd

_POS_BITS = 40                  # key = file index << 40 | byte offset: files up to 1 TiB, 2^23 reference files


def _key(file_idx, pos):
    return (int(file_idx) << _POS_BITS) | int(pos)


def _sites_of(total_deg_sites):
    """MapRef's match sites as _FileDriver renders them: the degenerate (0, "", "") sites lead (SmithWaterman.java:154,
    182-185; begin 0 sorts first, Distribution.java:428)"""
    _, deg, sites = total_deg_sites
    return [(0, ("", ""))] * deg + sites


def _crawl(root):
    c, out = _io.DirectoryCrawler(root), []
    while c.hasNext():
        out.append(c.next())
    return out


def run_rank(ctx, ref_dir, in_dir, out_dir, rank=0, world=1, delimiter=_io.DELIMITER, out_name="result", out_ext=".txt",
             params=None, stream_chunk_bytes=512 << 10, slots=0, parse_threads=0, reduce_device=None, group=None,
             obj_group=None, realign_pairs=1 << 22):
    """This rank's part of the driver over every reads file of `in_dir`; rank 0 writes the result files.  Returns the rank's
    stats: phase wall times (s), cells swept, records streamed per (reads file, reference file)."""
    import torch.distributed as dist
    from .aligner import make_params
    params = params if params is not None else make_params()
    ref_files, in_files = _crawl(ref_dir), _crawl(in_dir)
    st = {"rank": rank, "world": world, "parse_s": 0.0, "push_s": 0.0, "sweep_s": 0.0, "reduce_s": 0.0, "realign_s": 0.0,
          "gather_s": 0.0, "write_s": 0.0, "cells": 0, "records": 0, "winners_owned": 0, "files": []}
    for input_num, in_file in enumerate(in_files, 1):
        t0 = time.perf_counter()
        reads = _io.read_reads_packed(in_file, delimiter).sequences()          # InOutOps.java:60-88 (Distribution.java:313)
        t_exec = time.perf_counter()                                             # execTime starts here (:317)
        st["parse_s"] += t_exec - t0
        run_max, cands, n_local = 0, [], 0                                       # `int max = 0` (:323)
        per_file = []
        for fi, ref_file in enumerate(ref_files):
            ctx.set_option("scores_only", 1)                                     # (the slot contexts copy the options at open)
            ctx.set_option("stream_keep_records", 0)
            s = ctx.stream(reads, params, slots=slots, chunk_bytes=stream_chunk_bytes)
            try:
                a = time.perf_counter()
                s.push_file_shard(ref_file, rank, world, delimiter, parse_threads)
                b = time.perf_counter()
                s.finish()
                totals = s.totals()
                c = time.perf_counter()
                n = len(totals)
                stats = s.stats()
                st["push_s"] += b - a
                st["sweep_s"] += c - b
                st["cells"] += int(stats.cells)
                n_local += n
                per_file.append(n)
                fmax = int(totals.max()) if n else run_max
                if fmax >= run_max:                                              # candidates: this rank's running max with ties
                    if fmax > run_max:
                        run_max, cands = fmax, []
                    for r in np.flatnonzero(totals == run_max).tolist():
                        cands.append((_key(fi, s.ref_pos(r)), s.metadata(r), s.ref_sequence(r)))
            finally:
                s.close()
        ctx.set_option("scores_only", 0)
        st["records"] += n_local
        st["files"].append({"reads_file": input_num, "records_per_ref_file": per_file})

        t1 = time.perf_counter()
        keys = np.array([k for k, _, _ in cands], dtype=np.int64)
        best, winners = swd.global_max_with_ties(np.full(len(cands), run_max, dtype=np.int64), keys,
                                                 device=reduce_device, group=group)
        num_refs = n_local
        if world > 1:
            import torch
            cnt = torch.tensor([n_local], dtype=torch.int64)
            if reduce_device is not None:
                cnt = cnt.to(reduce_device)
            dist.all_reduce(cnt, group=group)                                    # `# Reference Sequences` (:331)
            num_refs = int(cnt.item())
        t2 = time.perf_counter()
        st["reduce_s"] += t2 - t1

        win = set(winners)
        own = [x for x in cands if x[0] in win]
        mine = []
        per_batch = max(1, realign_pairs // max(len(reads), 1))
        for lo in range(0, len(own), per_batch):
            part = own[lo:lo + per_batch]
            bt = ctx.upload([seq for _, _, seq in part], reads).run(params)      # the full path, winners only
            try:
                for (key, meta, seq), res in zip(part, bt.ref_sites_packed()):
                    if res[0] != best:
                        raise RuntimeError("reference %s: total %d on the full path, %d in the sweep" % (meta, res[0], best))
                    mine.append((key, meta, seq.decode("latin-1"), _sites_of(res)))
            finally:
                bt.free()
        st["winners_owned"] += len(mine)
        t3 = time.perf_counter()
        st["realign_s"] += t3 - t2

        if world > 1:
            got = [None] * world if rank == 0 else None
            dist.gather_object(mine, got, dst=0, group=obj_group)               # (pickles: never over RCCL)
        else:
            got = [mine]
        t4 = time.perf_counter()
        st["gather_s"] += t4 - t3
        if rank == 0:
            merged = sorted((x for part in got for x in part), key=lambda x: x[0])   # encounter order
            exec_ms = int((time.perf_counter() - t_exec) * 1000)                 # execTime ends before the sort (:358)
            opt = sorted((([meta, seq], sites) for _, meta, seq, sites in merged), key=lambda v: v[0][0])   # OptSeqsComp
            text = _io.InOutOps.GetOutputStr().call(reads, ((num_refs, len(reads)), best, exec_ms), opt)
            _io.InOutOps.PrintStrToFile().call("%s/%s%d%s" % (out_dir, out_name, input_num, out_ext), text)   # :364-365
        st["write_s"] += time.perf_counter() - t4
    return st


_ALIGN_MODES = {"local": _capi.ALIGN_LOCAL, "fit": _capi.ALIGN_FIT, "global": _capi.ALIGN_GLOBAL}


def _rank_main(args):
    """one rank of the CLI (a fresh child of the launcher)"""
    import torch
    import torch.distributed as dist
    import sparksmithwaterman_amd as sw
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    n_dev = torch.cuda.device_count()                     # (does not initialise the GPU)
    one_gpu = n_dev < world or os.environ.get("SWMI_ONE_GPU") == "1"
    dev_id = 0 if one_gpu else int(os.environ.get("LOCAL_RANK", rank))
    group = obj_group = None
    if world > 1:
        if one_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            torch.cuda.set_device(dev_id)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev_id))
            obj_group = dist.new_group(backend="gloo")
    tie = _capi.TIE_STRICT if args.tie == "strict" else _capi.TIE_SERIAL
    scores = [int(x) for x in args.scores.split(",")]
    ctx = sw.Context(dev_id)
    try:
        if len(scores) not in (3, 4, 6):                    # (the parser refuses it; a caller that builds args itself)
            raise ValueError("--scores takes 3, 4 or 6 entries, got %d" % len(scores))
        if len(scores) >= 4:                                # match,mismatch,gap,gapOpen: affine gaps on this rank's context
            ctx.set_option("gap_open", scores[3])
        if len(scores) == 6:                                # ...,gap2,gapOpen2: two-piece gaps (global and extend runs)
            ctx.set_option("gap2", scores[4])
            ctx.set_option("gap_open2", scores[5])
        scores = scores[:3]
        if args.align_mode != "local":                      # end-to-end alignment: the streamed scores-only pass and the
            ctx.set_option("align_mode", _ALIGN_MODES[args.align_mode])    # realignment of the winners both run on this context
        if args.long_reads:                                 # reads longer than 1024 bases on the affine kernels
            ctx.set_option("long_reads", 1)
        if args.band:                                       # ... inside a band around the diagonal
            ctx.set_option("band", args.band)
        if args.extend:                                     # seed extension: the global sweep, ended at the best cell
            ctx.set_option("extend", 1)
        if args.xdrop:                                      # ... with the drop-off rule for reads longer than 1024 bases
            ctx.set_option("xdrop", args.xdrop)
        if args.band_adapt:                                 # ... and the band re-centred on the alignment from strip to strip
            ctx.set_option("band_adapt", 1)
        if args.end_bonus:                                  # ... or a pair taken to the read's end when that is nearly as good
            ctx.set_option("end_bonus", args.end_bonus)
        if args.overlap:                                    # overlap alignment: the fit sweep with the read's ends free as well
            ctx.set_option("overlap", 1)
        if args.matrix:                                     # substitution scores on this rank's context (NCBI text format)
            from . import matrix as _matrix
            ctx.set_score_matrix(_matrix.load(args.matrix))
        t0 = time.perf_counter()
        st = run_rank(ctx, args.ref_dir, args.in_dir, args.out_dir, rank, world, args.delimiter, args.out_name, args.out_ext,
                      sw.make_params(scores, None, tie), args.stream_chunk_bytes, 0, 0,
                      reduce_device=None if (one_gpu or world == 1) else torch.device("cuda", dev_id),
                      group=group, obj_group=obj_group)
        st["total_s"] = time.perf_counter() - t0
    finally:
        ctx.close()
    st["backend"] = "none" if world == 1 else ("gloo" if one_gpu else "nccl")
    if args.stats:
        with open(args.stats.replace("<r>", str(rank)), "w") as f:
            json.dump(st, f)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _parser():
    import argparse

    class Parser(argparse.ArgumentParser):
        def parse_args(self, args=None, namespace=None):
            ns = super().parse_args(args, namespace)
            if len(ns.scores.split(",")) not in (3, 4, 6):
                self.error("--scores takes 3, 4 or 6 entries: match,mismatch,gap[,gapOpen[,gap2,gapOpen2]]")
            if ns.extend and ns.align_mode != "global":
                self.error("--extend requires --align-mode global")
            if ns.xdrop < 0 or ns.xdrop > _capi.XDROP_MAX:
                self.error("--xdrop takes a threshold of 0 .. 2^31 - 1")
            if ns.xdrop and not ns.extend:
                self.error("--xdrop requires --extend")
            if ns.band_adapt and not (ns.band and ns.extend):
                self.error("--band-adapt requires --band and --extend")
            if ns.end_bonus < 0 or ns.end_bonus > _capi.END_BONUS_MAX:
                self.error("--end-bonus takes a bonus of 0 .. 2^30")
            if ns.end_bonus and not ns.extend:
                self.error("--end-bonus requires --extend")
            if ns.end_bonus and (ns.xdrop or ns.band_adapt or len(ns.scores.split(",")) == 6):
                self.error("--end-bonus is not built for --xdrop, --band-adapt or two-piece gaps")
            if ns.overlap and ns.align_mode != "fit":
                self.error("--overlap requires --align-mode fit")
            if ns.overlap and (ns.band or len(ns.scores.split(",")) == 6):
                self.error("--overlap is not built for --band or two-piece gaps")
            return ns
    ap = Parser(description=__doc__.split("\n")[0])
    ap.add_argument("--ref-dir", required=True)
    ap.add_argument("--in-dir", required=True)
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--world", type=int, default=1)
    ap.add_argument("--delimiter", default=_io.DELIMITER)
    ap.add_argument("--out-name", default="result")
    ap.add_argument("--out-ext", default=".txt")
    ap.add_argument("--scores", default="5,-3,-4",
                    help="match,mismatch,gap (Distribution.java:36), match,mismatch,gap,gapOpen for affine gaps (gapOpen <= 0), or "
                         "match,mismatch,gap,gapOpen,gap2,gapOpen2 for two-piece gaps with --align-mode global: a gap of k bases costs "
                         "max(gapOpen + k * gap, gapOpen2 + k * gap2)")
    ap.add_argument("--matrix", default=None,
                    help="a substitution score matrix file in the NCBI text format (row = read base, column = reference base); "
                         "bases outside its alphabet score match / mismatch from --scores")
    ap.add_argument("--align-mode", choices=tuple(_ALIGN_MODES), default="local",
                    help="local: Smith-Waterman; fit: the whole read against any stretch of the reference; global: the whole read "
                         "against the whole reference.  Totals may then be zero or negative; the reduce keeps the control driver's "
                         "rule (`int max = 0`, ties kept): a reference whose total is negative never wins, and when no total is "
                         "positive the references whose total is exactly 0 tie, as they do today")
    ap.add_argument("--long-reads", action="store_true",
                    help="let the affine kernels (gapOpen, --matrix, --align-mode) take reads longer than 1024 bases, swept in strips "
                         "of 1024 rows (option long_reads); without it such a read is refused")
    ap.add_argument("--band", type=int, default=0, metavar="W",
                    help="with --long-reads: align a read longer than 1024 bases inside the band |j - i| <= W only, rounded outwards to "
                         "strips of 1024 rows (option band); runs on the affine kernels.  0 (the default): no band")
    ap.add_argument("--extend", action="store_true",
                    help="with --align-mode global: seed extension (option extend) -- the alignment is anchored at the start of the read "
                         "and of the reference and ends at the cell with the best score, the tails left unaligned; for left extension "
                         "reverse both sequences")
    ap.add_argument("--xdrop", type=int, default=0, metavar="X",
                    help="with --extend and --long-reads: the drop-off rule (option xdrop) -- the sweep of a read longer than 1024 bases "
                         "ends behind the first strip of 1024 rows whose last row lies more than X below the best score so far, and "
                         "the best cell so far is the answer.  0 (the default): off")
    ap.add_argument("--band-adapt", action="store_true",
                    help="with --band and --extend: the band follows the alignment (option band_adapt) -- the window of a strip of "
                         "1024 rows is placed around the column where the row above it scores best, so --band only has to cover the "
                         "drift inside one strip")
    ap.add_argument("--end-bonus", type=int, default=0, metavar="B",
                    help="with --extend: take a pair to the end of the read (option end_bonus) when the best extension that reaches it "
                         "scores less than B below the best one anywhere -- no soft clip for one mismatch near the read's end.  Not "
                         "with --xdrop, --band-adapt or two-piece gaps.  0 (the default): off")
    ap.add_argument("--overlap", action="store_true",
                    help="with --align-mode fit: overlap (ends-free) alignment (option overlap) -- the read's ends are free as well as the "
                         "reference's, and the alignment ends in the read's last row or the reference's last column.  Not with --band or "
                         "two-piece gaps")
    ap.add_argument("--tie", choices=("serial", "strict"), default="serial",
                    help="serial: SmithWaterman's aligner (NoDistribution, DistributeReference); strict: DistributedSW's (DistributeAlgorithm)")
    ap.add_argument("--stream-chunk-bytes", type=int, default=512 << 10, help="sequence bytes per streamed chunk")
    ap.add_argument("--stats", default=None, help="per-rank JSON of phase times, cells and records, e.g. O/rank<r>.json ('<r>': the rank)")
    return ap


def main(argv=None):
    import socket
    import subprocess
    import sys
    args = _parser().parse_args(argv)
    if "RANK" in os.environ:
        _rank_main(args)
        return 0
    # launcher: this process makes no GPU call; the ranks are fresh children (never a re-exec of a GPU process)
    os.makedirs(args.out_dir, exist_ok=True)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(args.world))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = [subprocess.Popen([sys.executable, "-m", "sparksmithwaterman_amd.sharded_files"] + (argv if argv is not None else sys.argv[1:]),
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(args.world)]
    rc = 0
    for p in procs:
        p.wait()
        rc = rc or p.returncode
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
