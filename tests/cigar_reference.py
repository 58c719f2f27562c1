"""The CIGAR contract of option "cigar" (include/swmi.h), restated -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  cigar(ref_aln, read_aln, mode) turns the two aligned strings of one alignment ('_' for
a gap, as every reference aligner of the tests returns them) into (entries, nm): entries = [(len, op_char), ...] from the start of
the alignment, adjacent entries never of the same op; a column whose reference string has '_' is I, one whose read string has '_'
is D, any other column is '=' when the two bases are equal after gotoh_reference.upper and X otherwise (mode 2), or M (mode 1).
nm = X columns + inserted + deleted bases, in both modes."""
import gotoh_reference as gr

GAP = gr.GAP_CHAR


def cigar(ref_aln, read_aln, mode=2):
    assert mode in (1, 2) and len(ref_aln) == len(read_aln)
    entries, nm = [], 0
    for r, q in zip(ref_aln, read_aln):
        assert not (r == GAP and q == GAP)
        if r == GAP:
            op = "I"
        elif q == GAP:
            op = "D"
        else:
            op = "=" if gr.upper(r) == gr.upper(q) else "X"
        nm += op != "="
        if mode == 1 and op in "=X":
            op = "M"
        if entries and entries[-1][1] == op:
            entries[-1] = (entries[-1][0] + 1, op)
        else:
            entries.append((1, op))
    return entries, nm
