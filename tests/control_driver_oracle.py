"""The control driver's loop with a selectable aligner -- TEST INFRASTRUCTURE ONLY, built from the unchanged pieces of
oracle/io_oracle_py.py and oracle/sw_oracle.py.

tie_mode=TIE_SERIAL is io_oracle_py.no_distribution (NoDistribution, src/sw/Distribution.java:482-634).  tie_mode=TIE_STRICT is
the same loop with DistributedSW's aligner and match-site sort, the same reduce (`int max = 0`, ties kept) and the same writer:
what DistributeAlgorithm runs (Distribution.java:140-210)."""
from oracle import io_oracle_py as ioo
from oracle import sw_oracle as orc


def control_driver(ref_dir, in_dir, delimiter, out_dir, out_name="result", out_ext=".txt",
                   scores=(5, -3, -4), types=b"aid-", tie_mode=orc.TIE_SERIAL):
    """Returns the list of result-file texts (also written to out_dir), Execution Time 0."""
    texts = []
    for input_num, in_file in enumerate(ioo._files_sorted(in_dir), 1):
        reads = ioo.get_reads(in_file, delimiter)
        num_refs, mx, opt = 0, 0, []
        for ref_file in ioo._files_sorted(ref_dir):
            ref_seqs = ioo.get_ref_seqs(ref_file, delimiter)
            num_refs += len(ref_seqs)
            for ref in ref_seqs:
                total, (_, sites) = orc.map_ref(ref, reads, scores, types, tie_mode)
                if total > mx:
                    mx, opt = total, [(ref, sites)]
                elif total == mx:
                    opt.append((ref, sites))
        opt.sort(key=lambda t: t[0][0])                        # OptSeqsComp, stable (:647-666)
        text = ioo.get_output_str(reads, (num_refs, len(reads)), mx, 0, opt)
        with open("%s/%s%d%s" % (out_dir, out_name, input_num, out_ext), "w", newline="", encoding="latin-1") as f:
            f.write(text)
        texts.append(text)
    return texts
