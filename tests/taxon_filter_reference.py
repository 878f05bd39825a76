"""Independent statement of the taxon filters (include/blu_pipeline.h: blu_taxon_filter), written with nothing
but `json.load`, `str.split` and `str.startswith`.  Test infrastructure in the manner of tests/hit_filter_reference.py: it
reads the `*.blutils.json` itself and shares no code with the library.

The rule under test: a run under a taxon filter gives what the run without it gives on `filter_text`'s copy of the table.
"""
import json

RANKS = {"u": "u", "undefined": "u", "d": "d", "domain": "d", "k": "k", "kingdom": "k", "p": "p", "phylum": "p", "c": "c",
         "class": "c", "o": "o", "order": "o", "f": "f", "family": "f", "g": "g", "genus": "g", "s": "s", "species": "s"}
NOT_ONLY = 0xFFFF


def norm_rank(rank: str) -> str:
    low = rank.strip().lower()
    return RANKS.get(low, low)          # (the test databases use the nine ranks only: no slug rule is restated here)


def lineage_elements(lineage: str):
    """[(rank, identifier)] of a lineage string; [] when any element is not exactly two parts around `__` (a bad lineage, which
    an empty string is too)."""
    out = []
    for el in lineage.split(";"):
        parts = el.split("__")
        if len(parts) != 2:
            return []
        out.append((norm_rank(parts[0]), parts[1]))
    return out


class Taxonomy:
    def __init__(self, db_path, use_taxid=False):
        key = "numericLineage" if use_taxid else "textLineage"
        self.elements = {}                                   # taxid -> elements of its FIRST listing
        self.nodes = set()                                   # every element of every listing that is not refused
        for t in json.load(open(db_path))["taxonomies"]:
            els = lineage_elements(t[key])
            self.elements.setdefault(int(t["taxid"]), els)
            self.nodes.update(els)

    def element(self, element: str):
        """element text -> (rank, identifier or prefix, is a pattern); ValueError when it is malformed or names no node"""
        parts = element.split("__")
        if len(parts) != 2 or not parts[0] or not parts[1]:
            raise ValueError(f"malformed element {element!r}")
        rank, ident = norm_rank(parts[0]), parts[1]
        if ident.endswith("*"):
            if not any(n[0] == rank and n[1].startswith(ident[:-1]) for n in self.nodes):
                raise ValueError(f"unknown element {element!r}")
            return rank, ident[:-1], True
        if (rank, ident) not in self.nodes:
            raise ValueError(f"unknown element {element!r}")
        return rank, ident, False

    @staticmethod
    def first_match(els, elements):
        """index of the first of `elements` (list order) that one of the lineage's elements `els` is, or None.  (Exact
        elements through a dict so that a list of 65 534 stays quick; the patterns one by one.)"""
        exact = {}
        for k, (rank, ident, pattern) in enumerate(elements):
            if not pattern:
                exact.setdefault((rank, ident), k)
        hits = [exact[n] for n in els if n in exact]
        hits += [k for k, (rank, pre, pattern) in enumerate(elements) if pattern and any(n[0] == rank and n[1].startswith(pre) for n in els)]
        return min(hits) if hits else None

    def code(self, taxid, exclude, only):
        """0 passes; k: the first exclude element (k - 1) the lineage holds; NOT_ONLY: fails the only list alone"""
        els = self.elements.get(taxid, [])
        k = self.first_match(els, exclude)
        if k is not None:
            return k + 1
        if only and self.first_match(els, only) is None:
            return NOT_ONLY
        return 0


def filter_text(src, dst, db_path, exclude=(), only=(), use_taxid=False, keep=None):
    """Copies the lines of `src` that pass (and that keep(fields), a threshold predicate, accepts) to `dst` verbatim; returns
    the counts over non-empty lines: n_lines, n_excluded, n_not_only, excluded_by, n_kept."""
    tax = Taxonomy(db_path, use_taxid)
    ex, on = [tax.element(e) for e in exclude], [tax.element(e) for e in only]
    codes = {}
    data = open(src, "rb").read()
    out, c = [], {"n_lines": 0, "n_excluded": 0, "n_not_only": 0, "excluded_by": [0] * len(ex), "n_kept": 0}
    pos = 0
    while pos < len(data):
        nl = data.find(b"\n", pos)
        end = len(data) if nl < 0 else nl + 1
        raw = data[pos:end]
        pos = end
        body = raw[:-1] if raw.endswith(b"\n") else raw
        if body.endswith(b"\r"):
            body = body[:-1]
        if not body:
            out.append(raw)
            continue
        c["n_lines"] += 1
        fields = body.split(b"\t")
        taxid = int(fields[2])
        if taxid not in codes:
            codes[taxid] = tax.code(taxid, ex, on)
        code = codes[taxid]
        if code == NOT_ONLY:
            c["n_not_only"] += 1
        elif code:
            c["n_excluded"] += 1
            c["excluded_by"][code - 1] += 1
        if code == 0 and (keep is None or keep(fields)):
            c["n_kept"] += 1
            out.append(raw)
    open(dst, "wb").write(b"".join(out))
    return c


# ---- a small database: 40 taxids over three domain-level clades ------------------------------------------------------------------
FIRST_TAXID, N_TAXIDS, N_UNKNOWN = 1000, 40, 5          # the tables also name taxids 1040 .. 1044, which the DB lacks
BAD_TAXID, EMPTY_TAXID = 1017, 1029


def _entries():
    tx = []
    for i in range(N_TAXIDS):
        taxid = FIRST_TAXID + i
        dom, dom_id = (("Bacteria", 2), ("Archaea", 2157), ("Eukaryota", 2759))[i % 3]
        fam = i % 3 * 10 + i // 3 % 4
        if i % 8 == 5:
            species = "uncultured-" + ("bacterium", "archaeon", "eukaryote")[i % 3]
        elif i % 8 == 2:
            species = "uncultured-organism"
        else:
            species = f"{dom[:3].lower()}-sp{i}"
        rank_s = "species" if i % 5 == 0 else "s"                  # (lineages spell ranks either way: one node)
        text = f"d__{dom};p__{dom[0]}phylum{i % 2};f__Fam{fam};g__Gen{i // 2};{rank_s}__{species}"
        numeric = f"d__{dom_id};p__{dom_id * 10 + i % 2};f__{5000 + fam};g__{7000 + i // 2};{rank_s}__{taxid}"
        if i % 3 == 2 and i % 4 == 3:
            text = text.replace("f__", "o__Chloroplast;f__")
            numeric = numeric.replace("f__", "o__4444;f__")
        if taxid == BAD_TAXID:                                      # one element of three parts: the whole lineage is refused
            text, numeric = f"d__{dom};p__only-here;c__x__y;s__lost", f"d__{dom_id};p__99;c__1__2;s__{taxid}"
        if taxid == EMPTY_TAXID:
            text = numeric = ""
        tx.append({"taxid": taxid, "rank": "species", "numericLineage": numeric, "textLineage": text, "accessions": []})
    return tx


def write_db(path, duplicate=None):
    """duplicate = (taxid, text lineage, numeric lineage): that taxid listed a second time at the end, with another lineage"""
    tx = _entries()
    if duplicate is not None:
        tx.append({"taxid": duplicate[0], "rank": "species", "numericLineage": duplicate[2], "textLineage": duplicate[1],
                   "accessions": []})
    open(path, "w").write(json.dumps({"blutilsVersion": "x", "sourceDatabase": "y", "taxonomies": tx}))
    return str(path)


E_FORMS = ["0.0", "1e-05", "3e-180", "2.5e-31", "1e-30", "7e-51", "1e-50", "0.001", "1e-100"]


def make_rows(n_q, hits, rng, long_names=False, sample_names=False, taxids=None, exact=False):
    """BLAST-shaped lines over the small database's taxids (the unknown ones included), columns 3, 4, 11 and 12 varying as in
    tests/hit_filter_reference.make_rows: 1 .. hits lines per query, or exactly `hits`.  taxids: draw from this list instead."""
    pool = list(taxids) if taxids is not None else list(range(FIRST_TAXID, FIRST_TAXID + N_TAXIDS + N_UNKNOWN))
    rows = []
    for q in range(n_q):
        if long_names:
            name = f"query_with_a_very_long_identifier_for_the_general_form_of_the_parse_kernel_{q:07d}/1_" + "x" * 60
        elif sample_names:
            name = f"s{q % 3}.{q}"
        else:
            name = f"q{q:06d}"
        for j in range(hits if exact else int(rng.integers(1, hits + 1))):
            t = pool[int(rng.integers(0, len(pool)))]
            bs = int(rng.integers(50, 200000))
            bs_txt = f"{bs}.5" if j % 5 == 0 else str(bs)
            ev = E_FORMS[int(rng.integers(0, len(E_FORMS)))]
            rows.append(f"{name}\tNR_{t:06d}.{j % 3}\t{t}\t{80 + int(rng.integers(0, 20001)) / 1000:.3f}\t{int(rng.integers(100, 2000))}"
                        f"\t1\t0\t1\t400\t1\t400\t{ev}\t{bs_txt}")
    return rows


def line(q, taxid, pid="99.0", aln="400", ev="1e-50", bs="700", acc=None):
    return f"{q}\t{acc or f'A{taxid}.1'}\t{taxid}\t{pid}\t{aln}\t0\t0\t1\t400\t1\t400\t{ev}\t{bs}"


# lists that cut the small database's tables: some lines excluded, some not in the only list, some kept
EXCLUDE = ["s__uncultured-*", "o__Chloroplast"]
ONLY = ["d__Bacteria", "d__Archaea"]
EXCLUDE_NUMERIC = ["o__4444", "s__1005", "g__700*"]
ONLY_NUMERIC = ["d__2", "d__2157"]
