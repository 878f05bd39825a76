"""Writes the taxdump fixture of the worked example in the reference book (docs/book/01_create_blutils_database.md:179-213):
the two species it prints, their ancestors with the ranks and the scientific names whose slugs are the printed text
lineages, the root, and the two blastdbcmd lines.  NCBI syntax: fields joined by "\\t|\\t", lines ending in "\\t|\\n";
taxidlineage.dmp lists the ancestors without the root, as NCBI's does.  Run from anywhere; writes next to this file."""
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# taxid, parent, rank, scientific name
NODES = [
    (1, 1, "no rank", "root"),
    (131567, 1, "no rank", "cellular organisms"),
    (2, 131567, "superkingdom", "Bacteria"),
    (200940, 2, "phylum", "Thermodesulfobacteriota"),
    (3024418, 200940, "class", "Desulfobacteria"),
    (213118, 3024418, "order", "Desulfobacterales"),
    (3031627, 213118, "family", "Desulfatibacillaceae"),
    (218207, 3031627, "genus", "Desulfatibacillum"),
    (259354, 218207, "species", "Desulfatibacillum alkenivorans"),
    (200918, 2, "phylum", "Thermotogota"),
    (188708, 200918, "class", "Thermotogae"),
    (1643947, 188708, "order", "Petrotogales"),
    (1643949, 1643947, "family", "Petrotogaceae"),
    (1511648, 1643949, "genus", "Defluviitoga"),
    (1006576, 1511648, "species", "Defluviitoga tunisiensis"),
]
ACCESSIONS = [("NR_025795.1", 259354, 1878), ("NR_122085.1", 1006576, 13670)]


def line(*fields):
    return "\t|\t".join(str(f) for f in fields) + "\t|\n"


def main():
    parent = {t: p for t, p, _, _ in NODES}
    def ancestors(t):
        out = []
        while parent[t] != t:
            t = parent[t]
            out.append(t)
        return [a for a in reversed(out) if a != 1]
    files = {
        "nodes.dmp": "".join(line(t, p, r, "", 0, 1, 11, 1, 0, 1, 0, 0, "") for t, p, r, _ in NODES),
        "names.dmp": "".join(line(t, n, "", "scientific name") for t, _, _, n in NODES),
        "taxidlineage.dmp": "".join(line(t, "".join(f"{a} " for a in ancestors(t))) for t, _, _, _ in NODES),
        "merged.dmp": "",
        "delnodes.dmp": "",
        "accessions.txt": "".join(f"{a}  {t}  {o}\n" for a, t, o in ACCESSIONS),
    }
    for name, text in files.items():
        with open(os.path.join(HERE, name), "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
