"""The SAM text of `sahara search --sam` (docs/semantics.md "SAM output") in
plain Python, from the kept rows and links of tests/pair_links_model.py and
the alignments of tests/align_model.py: the checker of the CLI's writer.
Shares no code with sahara_amd/cli."""
import numpy as np

import align_model as am
from pair_links_model import PRIMARY

LETTERS = {5: "$ACGT", 6: "$ACGNT"}  # rank -> letter (dna4, dna5)


def header(records):
    lines = ["@HD\tVN:1.6\tSO:unsorted\tGO:query"]
    lines += [f"@SQ\tSN:{i}\tLN:{len(r)}" for i, r in enumerate(records)]
    lines.append("@PG\tID:sahara\tPN:sahara")
    return "".join(ln + "\n" for ln in lines)


def sam_text(records, pats, sigma, kept, links, n_pairs, K, edit=True):
    """records: the index's records as ranks; pats: the interleaved patterns
    (qid i = row i: a read, then its reverse complement); kept, links: the
    model's rows and links; K: the alignment bound, max(-e, --rescue)."""
    T = am.concat_text(records)
    starts = np.concatenate([[0], np.cumsum([len(r) + 1 for r in records])])
    m = pats.shape[1]
    letters = LETTERS[sigma]

    def seq(qid):
        return "".join(letters[int(x)] for x in pats[qid])

    aligned = []
    for q, s, p, e in kept.tolist():
        res = am.align(pats[q].tolist(), T, int(starts[s]) + p, K, edit)
        assert res is not None, (q, s, p, e)
        aligned.append(res)
    out = [header(records)]
    by_pair = {}
    for i, q in enumerate(kept[:, 0].tolist()):
        by_pair.setdefault(q >> 2, []).append(i)
    for P in range(n_pairs):
        if P not in by_pair:
            for flag, qid in ((77, 4 * P), (141, 4 * P + 2)):
                out.append(f"{P}\t{flag}\t*\t0\t0\t*\t*\t0\t0\t{seq(qid)}\t*\n")
            continue
        for i in by_pair[P]:
            q, s, p, _ = kept[i].tolist()
            L = links[i]
            j = i + int(L["mate"])
            pm = int(kept[j, 2])
            flag = 0x1 | 0x2 | (0x10 if q & 1 else 0x20) | (0x80 if q & 2 else 0x40) | \
                (0 if L["flags"] & PRIMARY else 0x100)
            e_star, ref_len, edits = aligned[i]
            span = max(p + ref_len, pm + aligned[j][1]) - min(p, pm)
            left = p < pm or (p == pm and q % 2 == 0)
            out.append("\t".join(str(x) for x in (
                P, flag, s, p + 1, int(L["mapq"]), am.cigar(edits, m), "=", pm + 1, span if left else -span, seq(q),
                "*", f"NM:i:{e_star}", f"ZP:i:{int(L['score'])}")) + "\n")
    return "".join(out)
