"""bmx -- MI355X-native Boyer-Moore exact string matching.

A from-scratch gfx950 implementation of the one data-parallel hot path of
AnupBS28/PARALLEL_IMPLEMENTATION_OF_STRING_MATCHING_ALGORITHMS_OPENCL (its
``BoyreMoore/`` program), behind a C ABI (``include/bmx.h`` -> ``lib/libbmx.so``).

    host.py    ctypes binding of the C ABI (the product's Python face; no CPU fallback)
    corpus.py  synthetic corpora of BASELINE.json's configs (host numpy + in-HBM generator)
    shard.py   one-process-per-GPU sharding and the all-gatherv of match offsets
    csrc/      HIP kernels, the C-ABI shim, the host table builder, the C++ driver
"""
from . import corpus, host, shard  # noqa: F401
from .host import (BmxError, CLASS_ICASE, CLASS_IUPAC, Context, Dictionary, GAPS_LONGEST, GAPS_PROSITE, Index,  # noqa: F401
                   MAX_CLASS_PATTERN, MAX_GAPS_PATTERN, MAX_HAMMING_K, MAX_HAMMING_PATTERN, MAX_REGEX_POSITIONS, MAX_REGEX_STAR_WINDOW, REGEX_LONGEST,
                   REGEX_UNBOUNDED, ROW_NONE, ROWS_INVERT, Regex, Rows,
                   align, build_tables, cigar_strings, compile_classes, compile_gaps, compile_regex, compile_regex_star, edit_distance_batch,
                   grep, index_count, index_map, index_seeds, lcp_array, longest_repeat, rows_split, search, search_approx, search_classes,
                   search_dict, search_gaps, search_hamming, search_ranges, search_regex, search_regex_star)
from .host import reverse_regex, search_regex_begins, search_regex_star_begins  # noqa: F401
from .host import MAX_REGEX_LONG_POSITIONS, RegexLong, compile_regex_long, search_regex_long, widen_regex  # noqa: F401
from .host import REGEX_LINE, REGEX_WORD, RegexAnchors, compile_regex_anchored, search_regex_anchored  # noqa: F401
from .host import (EXPAND_EXTRACT, MAX_REGEX_GROUPS, MAX_TEMPLATE_REFS, RegexGroups, Template, compile_regex_groups,  # noqa: F401
                   compile_template, search_regex_groups)

__version__ = "0.1.0"
