// The label of one taxonomy row for `build-db sintax` and `build-db dada2` (DESIGN.md "Labelled FASTA export").  Neither
// format is in the reference: SINTAX headers are those of the usearch / vsearch manuals (`;tax=d:...,p:...;`), DADA2's
// those of assignTaxonomy's training files (`Level1;Level2;...;`).  Plain host code: tests/test_seqdb_label.py holds it
// against the restatement through blu_seqdb_render_labels.
#include "seqdb_labels.h"

#include "blu_internal.h"
#include "blu_pipeline.h"

namespace blu {

namespace {

// `,` and `:` are SINTAX's separators, `;` is both formats', white space would end the FASTA identifier
void put_ident(std::string_view ident, std::string* out) {
    for (unsigned char c : ident)
        out->push_back((c == ',' || c == ';' || c == ':' || c == ' ' || (c >= 9 && c <= 13)) ? '_' : (char)c);
}

}  // namespace

bool render_label(const LabelElement* el, size_t n, int format, std::string* out) {
    static const char letter[K_SPECIES + 1] = {0, 'd', 'k', 'p', 'c', 'o', 'f', 'g', 's'};
    size_t first[K_SPECIES + 1];                         // of two elements of one kind the first counts
    for (size_t& f : first) f = n;
    for (size_t i = 0; i < n; ++i) {
        if (el[i].rank_empty || el[i].ident.empty()) return false;
        const uint32_t k = el[i].kind;
        if (k >= K_DOMAIN && k <= K_SPECIES && first[k] == n) first[k] = i;
    }
    const size_t before = out->size();
    if (format == BLU_SEQDB_SINTAX) {                    // the kinds present, in lineage order
        for (size_t i = 0; i < n; ++i) {
            const uint32_t k = el[i].kind;
            if (k < K_DOMAIN || k > K_SPECIES || first[k] != i) continue;
            if (out->size() != before) out->push_back(',');
            out->push_back(letter[k]);
            out->push_back(':');
            put_ident(el[i].ident, out);
        }
    } else {                                             // fixed levels, cut before the first one the lineage lacks
        const uint32_t level[6] = {first[K_DOMAIN] != n ? (uint32_t)K_DOMAIN : (uint32_t)K_KINGDOM, K_PHYLUM, K_CLASS, K_ORDER,
                                   K_FAMILY, K_GENUS};
        for (const uint32_t k : level) {
            if (first[k] == n) break;
            put_ident(el[first[k]].ident, out);
            out->push_back(';');
        }
    }
    return out->size() != before;
}

}  // namespace blu
