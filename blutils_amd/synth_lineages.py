"""Seeded lineage tables in the form `build-db lineages` reads (`ID<TAB>d__Bacteria; p__Proteobacteria; ...`), for the tests
and scripts/lineage_db_bench.py.  The lineages are the root-to-node paths of a random tree, so that lines share prefixes as
the lines of SILVA or Greengenes do; the knobs cover what makes the parser and the path dictionary take another branch."""
from __future__ import annotations

from typing import List, Optional

import numpy as np

RANKS = ("d", "p", "c", "o", "f", "g", "s")
_SYLLABLES = ("bac", "ter", "ia", "pro", "teo", "coc", "cus", "myc", "es", "spi", "ro", "chae", "lac", "to", "vib", "rio",
              "ales", "aceae", "ota", "sedis", "incertae")


def _name(rng: np.random.Generator) -> str:
    return "".join(_SYLLABLES[k] for k in rng.integers(0, len(_SYLLABLES), int(rng.integers(2, 5)))).capitalize()


def make_lineages(n_distinct: int, depth: int, rng: np.random.Generator) -> List[List[str]]:
    """n_distinct root-to-leaf paths of `depth` levels (`rank__Name`), pairwise different; names repeat under different
    parents (`g__Incertae_sedis` style), so that equal last elements do not mean equal taxa."""
    ranks = [RANKS[k] if k < len(RANKS) else f"clade{k}" for k in range(depth)]
    paths: List[List[str]] = []
    seen = set()
    while len(paths) < n_distinct:
        if paths and rng.random() < 0.9:
            base = paths[int(rng.integers(0, len(paths)))]
            keep = int(rng.integers(0, depth))                   # levels shared with an earlier path
        else:
            base, keep = [], 0
        path = list(base[:keep])
        for k in range(keep, depth):
            path.append(f"{ranks[k]}__{_name(rng) if rng.random() < 0.9 else 'Incertae_sedis'}")
        if tuple(path) not in seen:
            seen.add(tuple(path))
            paths.append(path)
    return paths


def write_table(path: str, n_lines: int, n_distinct: int, depth: int = 7, seed: int = 0, ragged: float = 0.0,
                empty: float = 0.0, greengenes: float = 0.0, noise: float = 0.0, header: bool = False,
                confidence: bool = False, crlf: bool = False) -> Optional[str]:
    """Writes n_lines data lines over n_distinct lineages of `depth` levels.
    ragged: share of lines cut at a random level; empty: share without any level; greengenes: share whose tail is spelled
    `g__; s__`; noise: share of lines respelled (blanks around `;` and `__`, upper-case ranks, `_` and capitals in names:
    the same taxon, other bytes); header / confidence / crlf: the QIIME header line, a third column, CR LF line ends."""
    rng = np.random.default_rng(seed)
    paths = make_lineages(n_distinct, depth, rng)
    pick = rng.integers(0, n_distinct, n_lines)
    kind = rng.random(n_lines)
    noisy = rng.random(n_lines) < noise
    cut = rng.integers(1, depth + 1, n_lines)
    end = "\r\n" if crlf else "\n"
    with open(path, "w", newline="") as f:
        if header:
            f.write("Feature ID\tTaxon" + ("\tConfidence" if confidence else "") + end)
        for i in range(n_lines):
            levels = paths[int(pick[i])]
            if kind[i] < empty:
                levels = []
            elif kind[i] < empty + ragged:
                levels = levels[:int(cut[i])]
            elif kind[i] < empty + ragged + greengenes:
                k = int(cut[i]) - 1
                levels = levels[:k] + [lv.split("__")[0] + "__" for lv in levels[k:]]
            if noisy[i]:
                levels = [lv.split("__")[0].upper() + " __ " + lv.split("__", 1)[1].replace("_", " ").upper() for lv in levels]
                text = " ;  ".join(levels) + " ;"
            else:
                text = "; ".join(levels)
            f.write(f"seq{i}.{int(pick[i])}\t{text}" + ("\t0.98" if confidence else "") + end)
    return path
