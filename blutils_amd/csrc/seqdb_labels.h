// The labels of `build-db sintax` / `build-db dada2` (DESIGN.md "Labelled FASTA export"): one per row of the taxonomies
// file, rendered on the host once per call.  render_label is the rule itself (seqdb_labels.cpp: no I/O, no device);
// load_label_set reads the taxonomies file with the consensus use-case's loader and applies it to every row (pipeline_taxdb.cpp).
#ifndef BLU_SEQDB_LABELS_H
#define BLU_SEQDB_LABELS_H

#include <cstddef>
#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

#include "ingest.h"

namespace blu {

// one lineage element: the kind of its rank (1..8 = d k p c o f g s, RankKind's values; 0 = not a kind) and its identifier
struct LabelElement { uint32_t kind; bool rank_empty; std::string_view ident; };

// appends the label of one lineage to *out; false (nothing appended): the label is empty
bool render_label(const LabelElement* el, size_t n, int format, std::string* out);

struct LabelSet {
    std::vector<int64_t> taxid;          // [n_rows] in file order
    std::vector<uint64_t> off;           // [n_rows] the label's first byte in blob
    std::vector<uint32_t> len;           // [n_rows] 0 = no label
    std::string blob;
    TaxidMap row_of;                     // taxid -> its first row
};

// BLU_OK or the loader's error (a cache of the other lineage flavour is BLU_ERR_INVALID_ARG)
int load_label_set(const char* taxonomies_file, bool use_taxid, int format, LabelSet& out);

}  // namespace blu
#endif
