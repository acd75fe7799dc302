// bmx_main.cpp -- C++ host driver over libbmx.so.
//
// Keeps the I/O contract of the reference's console program
// (BoyreMoore/BoyreMoore/BoyreMoore.cpp): a text file and a pattern file in
// (defaults are the reference's hard-coded names, :77 and :82), the shift
// tables built on the host (:150-190), the search repeated 10 times with the
// text already on the device and the mean time printed (:211, :258, :288-292,
// :314-315), per-range hit counts printed (:294-295).  What it does NOT keep:
// the echo of the whole text (:92), the lossy 2-way split at spaces (:94-141)
// as the default partition, and the per-iteration context/JIT (:217-256).
//
//   bmx_cli [--text F] [--pattern F] [--iters N] [--positions] [--max-print K]
//           [--ranges P]      reference-compatible mode: split at spaces into P
//                             inclusive ranges like BoyreMoore.cpp:94-141 and
//                             print the per-range counts of bmx_search_ranges
//           [--device D]
//   bmx_cli --edit-distance A B [--iters N]   the reference's second program (EditDistance-1.cpp:
//                             two strings from files -- it opens str1.txt twice, :94-95 -- the mean time
//                             of the runs and the distance, :358-383)
//   bmx_cli --suffix-array F [--lcp] [--iters N] [--max-print K]   its third (SuffixArrays.cpp: text from
//                             input.txt, :181; array printed, :155-161; mean time, :514).  With --lcp (no counterpart
//                             in the reference) the LCP array is computed as well (bmx_lcp_array): its first --max-print
//                             values follow the array's, and one more line gives the longest repeat (length and two
//                             positions), the number of distinct substrings and the LCP kernels' time
//   bmx_cli --approx K [--text F] [--pattern F] [--iters N] [--positions] [--max-print K]
//                             approximate search (no counterpart in the reference; a pattern of up to 512 bytes, through
//                             bmx_search_approx_long*): every end of a match
//                             with at most K edits, on the resident text; prints the hit count, the first
//                             and last ends with their distances and the mean time
//   bmx_cli --classes EXPR [--icase] [--iupac] [--text F] [--iters N] [--positions] [--max-print K]
//                             class-pattern search (no counterpart in the reference): EXPR is a fixed-length
//                             expression of bytes, `.`, `[...]` sets and `\xHH` escapes (bmx_compile_classes);
//                             --icase folds the case of ASCII letters, --iupac reads R Y S W K M B D H V N as
//                             nucleotide sets; prints the hit count, the first and last starts and the mean time.
//                             With --approx K: the ends within K edits of the class pattern, printed as --approx does
//   bmx_cli --hamming K [--must A-B[,C-D...]] [--pattern F | --classes EXPR [--icase] [--iupac]] [--text F] [--iters N]
//           [--positions] [--max-print K]
//                             k-mismatch search (no counterpart in the reference): every start of a window with at most
//                             K substitutions against the pattern or the class expression (bmx_search_hamming*), none of
//                             them at a position of --must (inclusive ranges of pattern positions, from 0; a single
//                             position is A); prints the hit count, the first and last starts with their distances and
//                             the mean time, and with --positions one `Start at : P (distance D)` line per hit
//   bmx_cli --gaps EXPR [--prosite] [--icase] [--iupac] [--text F] [--iters N] [--positions] [--max-print K] [--starts [--longest]]
//                             gapped pattern search (no counterpart in the reference): EXPR is a class expression whose
//                             elements may carry ? {a} {a,b} (bmx_compile_gaps), with --prosite the PROSITE form
//                             C-x(2,4)-[LIVM]-{P}; prints the hit count, the first and last ends and the mean time as
//                             --classes does for starts.  With --starts the start of every match as well
//                             (bmx_search_gaps_spans: the largest one, with --longest the smallest), and --positions
//                             then prints `start end` pairs
//   bmx_cli --regex EXPR [--icase] [--iupac] [--text F] [--iters N] [--positions] [--max-print K] [--starts [--longest]]
//                             regular-expression search (no counterpart in the reference): EXPR is a star-free regular
//                             expression, the elements of --classes with groups ( ), alternation | and ? {a} {a,b} on
//                             elements and groups (bmx_compile_regex); prints what --gaps prints, `regex matches: N` in
//                             place of `gapped matches: N`.  It goes with none of --gaps, --classes, --approx, --hamming
//   bmx_cli --regex EXPR --begins [--spans [--longest]] [--icase] [--iupac] [--text F] [--positions] [--max-print K]
//                             the mirror image (bmx_search_regex_begins): every START at which a match begins, each once;
//                             `regex match starts: N`, and with --positions one `Start at : P` line per start.  With
//                             --spans the end of every start as well (bmx_search_regex_begins_spans: the smallest one,
//                             with --longest the largest) and `Match at : S E` lines
//   bmx_cli --regex-anchored EXPR [--word] [--line] ...
//                             --regex with the zero-width atoms ^ $ \b \B \< \> in EXPR (bmx_compile_regex_anchored,
//                             bmx_search_regex_anchored*; outside the text counts as a line break); --word is grep -w, --line
//                             is grep -x.  It takes every companion of --regex: --starts, --longest, --begins, --spans,
//                             --lines, --invert, --posix, --replace, --only-matching
//   bmx_cli --regex-long EXPR [--icase] [--iupac] [--text F] [--iters N] [--positions] [--max-print K] [--starts [--longest]]
//                             --regex for an expression of up to 128 positions after expansion (bmx_compile_regex_long,
//                             bmx_search_regex_long*); it prints what --regex prints and takes --lines, --replace,
//                             --only-matching and --merge as --regex does, but neither --begins nor --posix, and goes with
//                             none of the other search flags
//   bmx_cli --regex-star EXPR [--icase] [--iupac] [--text F] [--iters N] [--positions] [--max-print K]
//           [--starts --window N [--longest]]
//                             the same with unbounded repetition: EXPR may use * + {a,} (bmx_compile_regex_star,
//                             bmx_search_regex_star*); a match of no fixed longest length prints `matches of A or more
//                             bytes`.  --starts needs --window N (1..65536): the start of the shortest (--longest: the
//                             longest) match of at most N bytes, 18446744073709551615 where there is none.  It goes with
//                             none of --regex, --gaps, --classes, --approx, --hamming
//   bmx_cli --regex-star EXPR --begins [--spans --window N [--longest]] [--icase] [--iupac] [--text F] [--positions] [--max-print K]
//                             what --regex EXPR --begins prints, for an expression with * + {a,}
//                             (bmx_search_regex_star_begins); with --spans the smallest (--longest: the largest) end among
//                             the matches of at most N bytes from every start, 18446744073709551615 where there is none
//                             (bmx_search_regex_star_begins_spans), and `clipped by the window of N bytes: C`, the starts
//                             whose longest match may be longer than N
//   bmx_cli --approx K --spans [--best] [--pattern F | --classes EXPR [--icase] [--iupac]] [--text F] [--max-print K]
//                             after what --approx prints: the span of every match (bmx_search_approx_spans), the total
//                             and one `start end dist` line per span (at most --max-print of them); --best keeps one
//                             span per occurrence (BMX_SPANS_BEST) instead of one per qualifying end; with --cigar
//                             (a string pattern only) each span line ends in one more column, the span's CIGAR
//                             (bmx_align: = X I D runs)
//   bmx_cli --dict F [--text F] [--iters N] [--positions] [--max-print K]
//                             dictionary search (no counterpart in the reference): every occurrence of every
//                             pattern of F, one per line as `grep -F -f` reads it (empty lines skipped), in
//                             one pass; prints the pair count, the first and last (position, pattern) pairs
//                             and the mean time
//   bmx_cli --edit-distance-batch FILE_A FILE_B [--limit T] [--iters N]
//                             batched edit distance (EditDistance-1.cpp:278-345 looped by the caller): the files
//                             paired line by line, a one-line FILE_A against every line of FILE_B; one distance per
//                             line on stdout (min(d, T + 1) with --limit), the mean time on stderr
//   bmx_cli --index-count PATTERNS_FILE --text F [--positions] [--iters N] [--max-print K]
//                             text index (no counterpart in the reference): the suffix array of the text and a
//                             directory built once (bmx_index_create_device), then every line of PATTERNS_FILE
//                             (empty lines skipped) counted in one call; one `pattern<TAB>count` line per pattern
//                             on stdout, with --positions followed by a third tab-separated field of its ascending
//                             offsets (at most --max-print of them, blank-separated); build and mean query time on stderr
//   bmx_cli --index-seeds QUERIES_FILE --text F --min-len L [--max-occ N]
//                             seeds of every line of QUERIES_FILE (empty lines skipped) in the text: the matches of at
//                             least L bytes that no other match inside the same query contains, with at most N
//                             occurrences (0 or absent: no limit), through bmx_index_seeds; one line
//                             `query qpos len count first` per seed in order of (query, position), `first` the smallest
//                             text offset of the seed, and a last line `seeds TOTAL`
//   bmx_cli --index-map READS_FILE --text F --min-len L --max-occ N --approx K
//                             where every line of READS_FILE (empty lines skipped) lies in the text within K edits, by
//                             extending its seeds of (L, N >= 1), through bmx_index_map; one line `query start end dist`
//                             per read (`query - - -` for a read that maps nowhere) and a last line
//                             `mapped M of COUNT, candidates TOTAL`; not together with --index-seeds; with --cigar
//                             each line of a mapped read ends in one more column, its CIGAR (bmx_align)
//           [--gpus G]        also run the search over G GPUs from this one process: devices, RCCL
//                             communicators and the text set up once (bmx_multi_*), `iters` searches on
//                             the resident shards, each list checked against the one-GPU list; then once
//                             through the host-buffer entry point bmx_search_multi
//   bmx_cli (--replace STR | --only-matching) [--merge] [--lines] [--out F] [--max-print K] with --pattern, --classes,
//           --gaps, --regex, --regex-star or --approx K
//                             the non-overlapping matches, left to right (bmx_spans_select; --merge: the regions of the
//                             union of the longest match of every end), replaced by STR (bmx_replace: the new text on
//                             stdout or in F, a total line on stderr: sed s/x/STR/g) or printed one per line
//                             (bmx_extract, at most --max-print of them: grep -o); with --lines a match that crosses a
//                             line break is left alone.  --posix (with --regex or --regex-star, without --merge): the leftmost-longest
//                             matches, as grep -o and sed take them -- every start with its longest end
//                             (bmx_search_regex_begins_spans; with --lines the longest end inside the start's line,
//                             bmx_regex_ends_device with a limit), then the same selection.  With --regex-star it needs
//                             --window N (bmx_search_regex_star_begins_spans, bmx_regex_star_ends_device) and fails, exit
//                             status 1, if some match may be longer than N bytes: it never prints a shorter one
//   bmx_cli --regex-groups EXPR (--spans | --replace TEMPLATE | --only-matching [--template T]) [--posix] [--lines] [--out F]
//                             --regex where ( ... ) captures and (?: ... ) does not (bmx_compile_regex_groups).  --spans: every
//                             match end with the start of its shortest (--posix: longest) match and the half-open span of
//                             every group, "-" where unset (bmx_search_regex_groups).  --replace: the selection of --regex
//                             (--posix, --lines as there), the groups of the matches taken (bmx_regex_groups_device) and the
//                             text with every match replaced by the expansion of TEMPLATE: literal bytes, \1..\9,
//                             \g<0>..\g<16>, \\ (bmx_expand: sed 's/\(..\)\(..\)/\2\1/g').  --only-matching: the expansion of
//                             T (default \g<0>) for every match, one per line
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "bmx.h"

namespace {

bool read_file(const std::string &path, std::string &out)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

// The reference's partition (BoyreMoore.cpp:94-141): words are maximal runs
// between single spaces; P ranges of numberOfWords / P words each, inclusive
// [start, end] with the separating space excluded; leftover words are dropped.
std::vector<int32_t> split_like_reference(const std::string &text, int P)
{
    std::vector<int32_t> word_len;
    int32_t cur = 0;
    for (char ch : text) {
        if (ch == ' ') {
            word_len.push_back(cur);
            cur = 0;
        } else {
            ++cur;
        }
    }
    word_len.push_back(cur);
    const size_t per = word_len.size() / (size_t)P;
    std::vector<int32_t> se;
    int64_t pos = 0;
    size_t w = 0;
    for (int r = 0; r < P; ++r) {
        int64_t start = pos, end = pos;
        for (size_t j = 0; j < per; ++j, ++w) end += word_len[w] + 1;
        se.push_back((int32_t)start);
        se.push_back((int32_t)(end - 2)); // last character of the last word
        pos = end;
    }
    return se;
}

// Lines of a file as one blob plus offsets (the Arrow layout of bmx_edit_distance_batch); the newlines are dropped and a
// last line needs none.
void split_lines(const std::string &text, std::string &blob, std::vector<uint64_t> &off)
{
    off.assign(1, 0);
    size_t pos = 0;
    while (pos < text.size()) {
        size_t nl = text.find('\n', pos);
        if (nl == std::string::npos) nl = text.size();
        blob.append(text, pos, nl - pos);
        off.push_back(blob.size());
        pos = nl + 1;
    }
}

// --cigar: the script of every span as a SAM CIGAR string (bmx_align; "" for an entry without an alignment)
bool cigar_strings(bmx_ctx *ctx, const std::string &text, uint64_t base_offset, const void *pat, uint64_t pat_bytes,
                   const uint64_t *pat_off, uint64_t pat_count, const std::vector<uint64_t> &start, const std::vector<uint64_t> &end,
                   int k, std::vector<std::string> &out)
{
    const uint64_t count = start.size(), room = count * (2 * (uint64_t)k + 1);
    std::vector<uint64_t> op_off(count + 1, 0);
    std::vector<uint32_t> ops(room ? room : 1);
    uint64_t total = 0;
    const int rc = bmx_align(ctx, text.data(), text.size(), base_offset, pat, pat_bytes, pat_off, pat_count, nullptr, start.data(),
                             end.data(), count, k, nullptr, op_off.data(), ops.data(), room, &total);
    if (rc != BMX_OK) {
        fprintf(stderr, "bmx_align failed: %d (%s)\n", rc, bmx_last_error());
        return false;
    }
    out.assign(count, std::string());
    for (uint64_t e = 0; e < count; ++e)
        for (uint64_t j = op_off[e]; j < op_off[e + 1]; ++j) out[e] += std::to_string(ops[j] >> 4) + "MIDNSHP=X"[ops[j] & 15u];
    return true;
}

} // namespace

int main(int argc, char **argv)
{
    std::string text_path = "inputEd.txt", pat_path = "input1Search.txt", ed_a, ed_b, sa_path, dict_path, edb_a, edb_b, class_expr, index_path, seeds_path, map_path;
    uint32_t limit = BMX_ED_NO_LIMIT, class_flags = 0;
    bool have_classes = false, have_gaps = false, gaps_starts = false, gaps_longest = false;
    std::string gaps_expr, regex_expr;
    bool have_regex = false, regex_star = false, regex_both = false;
    bool regex_anchored = false; // --regex-anchored EXPR [--word] [--line]
    bool regex_long = false;     // --regex-long EXPR: up to 128 positions
    bool regex_groups = false, have_template = false; // --regex-groups EXPR: ( captures, (?: does not; --template T with --only-matching
    std::string template_str = "\\g<0>";
    uint32_t anchor_flags = 0;
    uint32_t star_window = 0;
    bool regex_begins = false, begins_spans = false, begins_longest = false, posix = false; // --begins [--spans [--longest]], --posix
    int iters = 10, device = 0, ranges = 0, gpus = 0, approx_k = -1, hamming_k = -1;
    std::string must_spec;
    bool positions = false, spans = false, spans_best = false, with_lcp = false, cigar = false, lines_mode = false, lines_invert = false;
    bool have_replace = false, only_matching = false, select_merge = false; // --replace STR, --only-matching, --merge, --out F
    std::string replace_str, out_path;
    uint64_t max_print = 32;
    uint32_t min_len = 0, max_occ = 0;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto need = [&](const char *name) -> const char * {
            if (i + 1 >= argc) {
                fprintf(stderr, "%s needs a value\n", name);
                exit(2);
            }
            return argv[++i];
        };
        if (a == "--text") text_path = need("--text");
        else if (a == "--pattern") pat_path = need("--pattern");
        else if (a == "--iters") iters = atoi(need("--iters"));
        else if (a == "--device") device = atoi(need("--device"));
        else if (a == "--gpus") gpus = atoi(need("--gpus"));
        else if (a == "--ranges") ranges = atoi(need("--ranges"));
        else if (a == "--max-print") max_print = strtoull(need("--max-print"), nullptr, 10);
        else if (a == "--positions") positions = true;
        else if (a == "--approx") approx_k = atoi(need("--approx"));
        else if (a == "--hamming") hamming_k = atoi(need("--hamming"));
        else if (a == "--must") must_spec = need("--must");
        else if (a == "--spans") spans = true;
        else if (a == "--best") spans_best = true;
        else if (a == "--cigar") cigar = true;
        else if (a == "--lcp") with_lcp = true;
        else if (a == "--lines") lines_mode = true;
        else if (a == "--replace") have_replace = true, replace_str = need("--replace");
        else if (a == "--only-matching") only_matching = true;
        else if (a == "--merge") select_merge = true;
        else if (a == "--out") out_path = need("--out");
        else if (a == "--invert") lines_invert = true;
        else if (a == "--dict") dict_path = need("--dict");
        else if (a == "--index-count") index_path = need("--index-count");
        else if (a == "--index-seeds") seeds_path = need("--index-seeds");
        else if (a == "--index-map") map_path = need("--index-map");
        else if (a == "--min-len") min_len = (uint32_t)strtoul(need("--min-len"), nullptr, 10);
        else if (a == "--max-occ") max_occ = (uint32_t)strtoul(need("--max-occ"), nullptr, 10);
        else if (a == "--classes") class_expr = need("--classes"), have_classes = true;
        else if (a == "--gaps") gaps_expr = need("--gaps"), have_gaps = true;
        else if (a == "--regex") regex_both = have_regex, regex_expr = need("--regex"), have_regex = true;
        else if (a == "--regex-long") regex_both = have_regex, regex_expr = need("--regex-long"), have_regex = regex_long = true;
        else if (a == "--regex-star") regex_both = have_regex, regex_expr = need("--regex-star"), have_regex = regex_star = true;
        else if (a == "--regex-anchored") regex_both = have_regex, regex_expr = need("--regex-anchored"), have_regex = regex_anchored = true;
        else if (a == "--regex-groups") regex_both = have_regex, regex_expr = need("--regex-groups"), have_regex = regex_groups = true;
        else if (a == "--template") have_template = true, template_str = need("--template");
        else if (a == "--word") anchor_flags |= BMX_REGEX_WORD;
        else if (a == "--line") anchor_flags |= BMX_REGEX_LINE;
        else if (a == "--begins") regex_begins = true;
        else if (a == "--posix") posix = true;
        else if (a == "--window") star_window = (uint32_t)strtoul(need("--window"), nullptr, 10);
        else if (a == "--prosite") class_flags |= BMX_GAPS_PROSITE;
        else if (a == "--starts") gaps_starts = true;
        else if (a == "--longest") gaps_longest = true;
        else if (a == "--icase") class_flags |= BMX_CLASS_ICASE;
        else if (a == "--iupac") class_flags |= BMX_CLASS_IUPAC;
        else if (a == "--limit") limit = (uint32_t)strtoul(need("--limit"), nullptr, 10);
        else if (a == "--edit-distance-batch") {
            edb_a = need("--edit-distance-batch");
            edb_b = need("--edit-distance-batch");
        } else if (a == "--edit-distance") {
            ed_a = need("--edit-distance");
            ed_b = need("--edit-distance");
        } else if (a == "--suffix-array") sa_path = need("--suffix-array");
        else {
            fprintf(stderr, "unknown option %s\n", a.c_str());
            return 2;
        }
    }

    if (!map_path.empty() && !seeds_path.empty()) {
        fprintf(stderr, "--index-seeds and --index-map exclude each other\n");
        return 2;
    }
    if (!map_path.empty()) seeds_path = map_path; // the same query file, read below
    if (regex_begins) { // --spans and --longest are the begins search's here
        begins_spans = spans, begins_longest = gaps_longest;
        spans = gaps_longest = false;
        if (!have_regex || gaps_starts || posix || lines_mode || have_replace || only_matching || (begins_longest && !begins_spans)) {
            fprintf(stderr, "--begins needs --regex EXPR or --regex-star EXPR and goes with --spans [--longest], --positions and --max-print only\n");
            return 2;
        }
    }
    const bool groups_spans = regex_groups && spans; // --regex-groups EXPR --spans [--posix]: every match with its groups
    if (regex_groups && (regex_both || regex_begins || gaps_starts || select_merge || positions || lines_invert ||
                         (groups_spans ? (have_replace || only_matching || lines_mode) : !(have_replace || only_matching)))) {
        fprintf(stderr, "--regex-groups EXPR goes with --spans [--posix], or with --replace TEMPLATE or --only-matching [--template T] and "
                        "[--posix] [--lines] [--out F]\n");
        return 2;
    }
    if (have_template && !(regex_groups && only_matching)) {
        fprintf(stderr, "--template T goes with --regex-groups EXPR --only-matching\n");
        return 2;
    }
    if (posix && !groups_spans && (!have_regex || select_merge || !(have_replace || only_matching))) {
        fprintf(stderr, "--posix needs --regex EXPR or --regex-star EXPR with --replace STR or --only-matching, without --merge\n");
        return 2;
    }
    if ((spans && approx_k < 0 && !groups_spans) || (spans_best && !spans)) {
        fprintf(stderr, "--spans needs --approx K, --best needs --spans\n");
        return 2;
    }
    if (cigar && ((!spans && map_path.empty()) || have_classes)) {
        fprintf(stderr, "--cigar needs --approx K --spans with a string pattern, or --index-map\n");
        return 2;
    }

    uint64_t must = 0;
    if ((!must_spec.empty() && hamming_k < 0) || (hamming_k >= 0 && (approx_k >= 0 || have_gaps))) {
        fprintf(stderr, "--must needs --hamming K; --hamming goes with neither --approx nor --gaps\n");
        return 2;
    }
    for (const char *p = must_spec.c_str(); *p;) { // A-B[,C-D...]: inclusive ranges of positions
        char *end = nullptr;
        const unsigned long from = strtoul(p, &end, 10);
        unsigned long to = from;
        bool ok = end != p;
        if (ok && *end == '-') {
            p = end + 1;
            to = strtoul(p, &end, 10);
            ok = end != p;
        }
        if (!ok || to < from || to >= 64 || (*end != ',' && *end != 0) || (*end == ',' && end[1] == 0)) {
            fprintf(stderr, "bad --must %s\n", must_spec.c_str());
            return 2;
        }
        for (unsigned long i = from; i <= to; ++i) must |= 1ull << i;
        p = *end ? end + 1 : end;
    }

    if (regex_long && (regex_begins || posix)) {
        fprintf(stderr, "--regex-long goes with neither --begins nor --posix\n");
        return 2;
    }
    if (anchor_flags != 0 && !regex_anchored) {
        fprintf(stderr, "--word and --line go with --regex-anchored EXPR\n");
        return 2;
    }
    if (have_regex && (have_gaps || have_classes || approx_k >= 0 || hamming_k >= 0 || (class_flags & BMX_GAPS_PROSITE))) {
        fprintf(stderr, "--regex goes with none of --gaps, --prosite, --classes, --approx, --hamming\n");
        return 2;
    }
    const bool star_windowed = regex_star && (gaps_starts || begins_spans || posix); // what looks for a match's other end
    if (regex_both || (star_windowed && (star_window < 1 || star_window > BMX_MAX_REGEX_STAR_WINDOW)) || (star_window != 0 && !star_windowed)) {
        fprintf(stderr, "--regex-star goes without --regex; its --starts, its --begins --spans and its --posix need --window N with 1 <= N <= 65536, "
                        "and --window goes with nothing else\n");
        return 2;
    }
    if ((gaps_starts && !have_gaps && !have_regex) || ((class_flags & BMX_GAPS_PROSITE) && !have_gaps)) {
        fprintf(stderr, "--starts needs --gaps EXPR or --regex EXPR, --prosite needs --gaps EXPR\n");
        return 2;
    }
    if ((gaps_longest && !gaps_starts) || (have_gaps && (have_classes || approx_k >= 0))) {
        fprintf(stderr, "--longest needs --starts; --gaps goes with neither --classes nor --approx\n");
        return 2;
    }

    const bool subst_mode = have_replace || only_matching;
    if ((have_replace && only_matching) || ((select_merge || !out_path.empty()) && !subst_mode) || (subst_mode && lines_invert) ||
        replace_str.size() > BMX_MAX_REPLACEMENT) {
        fprintf(stderr, "--replace STR (at most 65536 bytes) or --only-matching, not both; --merge and --out F go with one of them, --invert with neither\n");
        return 2;
    }
    if ((lines_invert && !lines_mode) ||
        ((lines_mode || subst_mode) && (hamming_k >= 0 || spans || gaps_starts || positions || ranges > 0 || gpus > 0 || !dict_path.empty() ||
                        !index_path.empty() || !seeds_path.empty() || !sa_path.empty() || !ed_a.empty() || !edb_a.empty()))) {
        fprintf(stderr, "--invert needs --lines; --lines, --replace and --only-matching go with --pattern, --classes, --gaps, --regex, --regex-star and --approx K only\n");
        return 2;
    }

    if (!seeds_path.empty()) {
        std::string text, lines, raw, blob;
        std::vector<uint64_t> raw_off, off(1, 0);
        if (min_len == 0) {
            fprintf(stderr, "--index-seeds and --index-map need --min-len L with L >= 1\n");
            return 2;
        }
        if (!map_path.empty() && (max_occ == 0 || approx_k < 0 || approx_k > BMX_MAP_MAX_K)) {
            fprintf(stderr, "--index-map needs --max-occ N with N >= 1 and --approx K with 0 <= K <= %d\n", BMX_MAP_MAX_K);
            return 2;
        }
        if (!read_file(text_path, text) || !read_file(seeds_path, lines)) {
            fprintf(stderr, "File Not Found!\n");
            return 1;
        }
        split_lines(lines, raw, raw_off);
        for (size_t i = 0; i + 1 < raw_off.size(); ++i) { // empty lines skipped, a trailing \r dropped
            uint64_t b = raw_off[i], e = raw_off[i + 1];
            if (e > b && raw[e - 1] == '\r') --e;
            if (e == b) continue;
            blob.append(raw, b, e - b);
            off.push_back(blob.size());
        }
        const uint64_t count = off.size() - 1, n = text.size();
        if (count == 0) {
            fprintf(stderr, "no query in %s\n", seeds_path.c_str());
            return 1;
        }
        bmx_ctx *ctx = nullptr;
        int rc = bmx_ctx_create(device, &ctx);
        if (!map_path.empty()) {
            std::vector<uint64_t> start(count), end(count);
            std::vector<uint8_t> dist(count);
            uint64_t total = 0, mapped = 0;
            if (rc == BMX_OK)
                rc = bmx_index_map(ctx, text.data(), n, blob.data(), blob.size(), off.data(), count, min_len, max_occ, approx_k,
                                   start.data(), end.data(), dist.data(), nullptr, nullptr, nullptr, nullptr, 0, &total);
            if (rc != BMX_OK) {
                fprintf(stderr, "bmx_index_map failed: %d (%s)\n", rc, bmx_last_error());
                return 1;
            }
            std::vector<std::string> scripts;
            if (cigar && !cigar_strings(ctx, text, 0, blob.data(), blob.size(), off.data(), count, start, end, approx_k, scripts)) return 1;
            for (uint64_t q = 0; q < count; ++q) {
                if (dist[q] == BMX_MAP_NO_HIT) {
                    printf("%llu - - -\n", (unsigned long long)q);
                    continue;
                }
                printf("%llu %llu %llu %u", (unsigned long long)q, (unsigned long long)start[q], (unsigned long long)end[q], dist[q]);
                if (cigar) printf(" %s", scripts[q].c_str());
                printf("\n");
                ++mapped;
            }
            printf("mapped %llu of %llu, candidates %llu\n", (unsigned long long)mapped, (unsigned long long)count,
                   (unsigned long long)total);
            bmx_ctx_destroy(ctx);
            return 0;
        }
        std::vector<uint64_t> seed_off(count + 1, 0);
        std::vector<uint32_t> qpos, len, lo, cnt;
        std::vector<int32_t> sa(n);
        uint64_t total = 0;
        if (rc == BMX_OK) { // a counting call, then the list
            rc = bmx_index_seeds(ctx, text.data(), n, blob.data(), blob.size(), off.data(), count, min_len, max_occ, seed_off.data(),
                                 nullptr, nullptr, nullptr, nullptr, 0, &total);
            if (rc == BMX_ERR_CAPACITY) {
                qpos.resize(total), len.resize(total), lo.resize(total), cnt.resize(total);
                rc = bmx_index_seeds(ctx, text.data(), n, blob.data(), blob.size(), off.data(), count, min_len, max_occ,
                                     seed_off.data(), qpos.data(), len.data(), lo.data(), cnt.data(), total, &total);
            }
        }
        if (rc == BMX_OK && total > 0) rc = bmx_suffix_array(ctx, text.data(), n, sa.data()); // the array lo and cnt point into
        if (rc != BMX_OK) {
            fprintf(stderr, "bmx_index_seeds failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        for (uint64_t q = 0; q < count; ++q)
            for (uint64_t s = seed_off[q]; s < seed_off[q + 1]; ++s) {
                const int32_t first = *std::min_element(sa.begin() + lo[s], sa.begin() + lo[s] + cnt[s]);
                printf("%llu %u %u %u %d\n", (unsigned long long)q, qpos[s], len[s], cnt[s], first);
            }
        printf("seeds %llu\n", (unsigned long long)total);
        bmx_ctx_destroy(ctx);
        return 0;
    }

    if (!index_path.empty()) {
        std::string text, lines, raw, blob;
        std::vector<uint64_t> raw_off, off(1, 0);
        if (!read_file(text_path, text) || !read_file(index_path, lines)) {
            fprintf(stderr, "File Not Found!\n");
            return 1;
        }
        split_lines(lines, raw, raw_off);
        for (size_t i = 0; i + 1 < raw_off.size(); ++i) { // empty lines skipped, a trailing \r dropped
            uint64_t b = raw_off[i], e = raw_off[i + 1];
            if (e > b && raw[e - 1] == '\r') --e;
            if (e == b) continue;
            blob.append(raw, b, e - b);
            off.push_back(blob.size());
        }
        const uint64_t count = off.size() - 1, n = text.size();
        if (count == 0) {
            fprintf(stderr, "no pattern in %s\n", index_path.c_str());
            return 1;
        }
        bmx_ctx *ctx = nullptr;
        bmx_index *ix = nullptr;
        void *d_text = nullptr, *d_pat = nullptr, *d_off = nullptr, *d_cnt = nullptr;
        int rc = bmx_ctx_create(device, &ctx);
        if (rc == BMX_OK) rc = bmx_text_upload(ctx, text.data(), n, &d_text);
        if (rc == BMX_OK) rc = bmx_text_upload(ctx, blob.data(), blob.size(), &d_pat);
        if (rc == BMX_OK) rc = bmx_text_upload(ctx, (const char *)off.data(), off.size() * sizeof(uint64_t), &d_off);
        if (rc == BMX_OK) rc = bmx_device_alloc(ctx, (count + 1) * sizeof(uint32_t), &d_cnt);
        if (rc == BMX_OK) rc = bmx_index_create_device(ctx, d_text, n, nullptr, nullptr, &ix);
        if (rc != BMX_OK) {
            fprintf(stderr, "index setup failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        const float build_ms = bmx_index_build_ms(ix);
        double total = 0.0, kernel_ms = 0.0;
        if (iters < 1) iters = 1;
        for (int it = 0; it < iters; ++it) { // the timed calls: the resident index, results left on the device
            auto t0 = std::chrono::steady_clock::now();
            rc = bmx_index_count_device(ctx, ix, d_pat, blob.size(), (const uint64_t *)d_off, count, nullptr, (uint32_t *)d_cnt, nullptr);
            auto t1 = std::chrono::steady_clock::now();
            if (rc != BMX_OK) {
                fprintf(stderr, "bmx_index_count_device failed: %d (%s)\n", rc, bmx_last_error());
                return 1;
            }
            total += std::chrono::duration<double>(t1 - t0).count();
            kernel_ms += bmx_last_index_ms(ctx);
        }
        bmx_index_destroy(ix);
        for (void *p : {d_text, d_pat, d_off, d_cnt})
            if (p) bmx_device_free(ctx, p);
        // what is printed comes through the host-buffer entry points: (text, patterns) -> counts, positions
        std::vector<uint64_t> out_off(count + 1, 0), pos(1);
        uint64_t hits = 0;
        rc = bmx_index_locate(ctx, text.data(), n, blob.data(), blob.size(), off.data(), count, out_off.data(), nullptr, 0, &hits);
        if (rc == BMX_ERR_CAPACITY && positions) {
            pos.resize(hits);
            rc = bmx_index_locate(ctx, text.data(), n, blob.data(), blob.size(), off.data(), count, out_off.data(), pos.data(), hits, &hits);
        }
        if (rc != BMX_OK && rc != BMX_ERR_CAPACITY) {
            fprintf(stderr, "bmx_index_locate failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        for (uint64_t i = 0; i < count; ++i) {
            fwrite(blob.data() + off[i], 1, off[i + 1] - off[i], stdout);
            printf("\t%llu", (unsigned long long)(out_off[i + 1] - out_off[i]));
            if (positions) {
                printf("\t");
                for (uint64_t j = out_off[i]; j < out_off[i + 1] && j - out_off[i] < max_print; ++j)
                    printf(j == out_off[i] ? "%llu" : " %llu", (unsigned long long)pos[j]);
            }
            printf("\n");
        }
        fprintf(stderr, "Average time = %.6f s  (kernel %.3f ms, %llu patterns, %llu occurrences, index built in %.3f ms)\n",
                total / iters, kernel_ms / iters, (unsigned long long)count, (unsigned long long)hits, build_ms);
        bmx_ctx_destroy(ctx);
        return 0;
    }

    if (!edb_a.empty()) {
        std::string x, y, ablob, bblob;
        std::vector<uint64_t> aoff, boff;
        if (!read_file(edb_a, x) || !read_file(edb_b, y)) {
            fprintf(stderr, "File Not Found!\n");
            return 1;
        }
        split_lines(x, ablob, aoff);
        split_lines(y, bblob, boff);
        const uint64_t a_count = aoff.size() - 1, count = boff.size() - 1;
        if (a_count != 1 && a_count != count) {
            fprintf(stderr, "%llu lines against %llu: FILE_A needs one line or as many as FILE_B\n", (unsigned long long)a_count,
                    (unsigned long long)count);
            return 1;
        }
        bmx_ctx *ctx = nullptr;
        int rc = bmx_ctx_create(device, &ctx);
        if (rc != BMX_OK) {
            fprintf(stderr, "bmx_ctx_create failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        std::vector<uint32_t> dist(count ? count : 1);
        double total = 0.0, kernel_ms = 0.0;
        if (iters < 1) iters = 1;
        for (int it = 0; it < iters; ++it) {
            auto t0 = std::chrono::steady_clock::now();
            rc = bmx_edit_distance_batch(ctx, ablob.data(), ablob.size(), aoff.data(), a_count, bblob.data(), bblob.size(),
                                         boff.data(), count, limit, dist.data());
            auto t1 = std::chrono::steady_clock::now();
            if (rc != BMX_OK) {
                fprintf(stderr, "bmx_edit_distance_batch failed: %d (%s)\n", rc, bmx_last_error());
                return 1;
            }
            total += std::chrono::duration<double>(t1 - t0).count();
            kernel_ms += count ? bmx_last_ed_batch_ms(ctx) : 0.0;
        }
        for (uint64_t i = 0; i < count; ++i) printf("%u\n", dist[i]);
        fprintf(stderr, "Average time = %.6f s  (kernel %.3f ms, %llu pairs, %lld pair by pair)\n", total / iters, kernel_ms / iters,
                (unsigned long long)count, count ? (long long)bmx_last_ed_batch_fallbacks(ctx) : 0ll);
        bmx_ctx_destroy(ctx);
        return 0;
    }

    if (!ed_a.empty() || !sa_path.empty()) {
        bmx_ctx *ctx = nullptr;
        int rc = bmx_ctx_create(device, &ctx);
        if (rc != BMX_OK) {
            fprintf(stderr, "bmx_ctx_create failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        double total = 0.0;
        if (!ed_a.empty()) {
            std::string x, y;
            if (!read_file(ed_a, x) || !read_file(ed_b, y)) {
                fprintf(stderr, "File Not Found!\n"); // EditDistance-1.cpp:99
                return 1;
            }
            uint64_t d = 0;
            for (int it = 0; it < iters; ++it) {
                auto t0 = std::chrono::steady_clock::now();
                rc = bmx_edit_distance(ctx, x.data(), x.size(), y.data(), y.size(), &d);
                auto t1 = std::chrono::steady_clock::now();
                if (rc != BMX_OK) {
                    fprintf(stderr, "bmx_edit_distance failed: %d (%s)\n", rc, bmx_last_error());
                    return 1;
                }
                total += std::chrono::duration<double>(t1 - t0).count();
            }
            printf("%llu %llu\n", (unsigned long long)x.size(), (unsigned long long)y.size());
            printf("%llu\n", (unsigned long long)d);                                  // :369
            if (iters > 0) printf("\n\nAverage time :%f \n", total / iters);          // :383
        } else {
            std::string t;
            if (!read_file(sa_path, t)) {
                fprintf(stderr, "File Not Found!\n"); // SuffixArrays.cpp:185
                return 1;
            }
            std::vector<int32_t> sa(t.size() ? t.size() : 1), lcp;
            with_lcp = with_lcp && !t.empty(); // (an empty text has neither)
            if (with_lcp) lcp.resize(t.size());
            for (int it = 0; it < iters || (with_lcp && it == 0); ++it) {
                auto t0 = std::chrono::steady_clock::now();
                rc = with_lcp ? bmx_lcp_array(ctx, t.data(), t.size(), sa.data(), lcp.data())
                              : bmx_suffix_array(ctx, t.data(), t.size(), sa.data());
                auto t1 = std::chrono::steady_clock::now();
                if (rc != BMX_OK) {
                    fprintf(stderr, "%s failed: %d (%s)\n", with_lcp ? "bmx_lcp_array" : "bmx_suffix_array", rc, bmx_last_error());
                    return 1;
                }
                total += std::chrono::duration<double>(t1 - t0).count();
            }
            printf("%llu\n", (unsigned long long)t.size()); // :198
            for (uint64_t i = 0; i < t.size() && i < max_print; ++i) printf("%d ", sa[i]); // :158-160
            printf("\n");
            if (with_lcp) {
                uint64_t sum = 0, best = 0;
                for (uint64_t j = 0; j < lcp.size(); ++j) {
                    sum += (uint64_t)lcp[j];
                    if (lcp[j] > lcp[best]) best = j;
                }
                const uint64_t n = t.size();
                for (uint64_t i = 0; i < n && i < max_print; ++i) printf("%d ", lcp[i]);
                printf("\n");
                if (lcp[best] > 0) printf("Longest repeat = %d at %d and %d", lcp[best], sa[best - 1], sa[best]);
                else printf("Longest repeat = 0");
                printf(", distinct substrings = %llu, LCP kernels = %f ms\n", (unsigned long long)(n * (n + 1) / 2 - sum),
                       bmx_last_lcp_ms(ctx));
            }
            if (iters > 0) printf("Average Time  = %f\n", total / iters); // :514
        }
        bmx_ctx_destroy(ctx);
        return 0;
    }

    std::string text, pat;
    if (!read_file(text_path, text)) {
        fprintf(stderr, "cannot read text file %s\n", text_path.c_str());
        return 1;
    }
    if (dict_path.empty() && !have_classes && !have_gaps && !have_regex && !read_file(pat_path, pat)) { // (a dictionary search reads its own list, a class search its expression)
        fprintf(stderr, "cannot read pattern file %s\n", pat_path.c_str());
        return 1;
    }
    const uint64_t n = text.size();
    int32_t m = (int32_t)pat.size();
    std::vector<uint8_t> classes(BMX_MAX_CLASS_PATTERN * BMX_CLASS_BYTES);
    if (have_classes && bmx_compile_classes(class_expr.data(), class_expr.size(), class_flags, classes.data(), &m) != BMX_OK) {
        fprintf(stderr, "bad class expression %s\n", class_expr.c_str());
        return 1;
    }
    uint64_t gaps_optional = 0;
    if (have_gaps && bmx_compile_gaps(gaps_expr.data(), gaps_expr.size(), class_flags, classes.data(), &gaps_optional, &m) != BMX_OK) {
        fprintf(stderr, "bad gapped pattern expression %s\n", gaps_expr.c_str());
        return 1;
    }
    // --lines: the rows of the text that hold a match (or, --invert, none): row<TAB>count, 0-based.  --replace STR and
    // --only-matching: the non-overlapping matches (--merge: the regions of their union, from the longest match of every end)
    // replaced by STR, or one per line; with --lines a match that crosses a line break is left alone.
    // --regex-groups EXPR --spans: every end at which a match ends with the start of its shortest (--posix: longest) match and
    // the half-open span of every group, "-" for a group that is unset
    if (groups_spans) {
        bmx_regex re;
        std::unique_ptr<bmx_regex_groups> gr(new bmx_regex_groups);
        if (bmx_compile_regex_groups(regex_expr.data(), regex_expr.size(), class_flags, &re, gr.get()) != BMX_OK) {
            fprintf(stderr, "bad regular expression %s (%s)\n", regex_expr.c_str(), bmx_last_error());
            return 1;
        }
        const uint64_t room = n ? n : 1, pairs = (uint64_t)gr->n_groups + 1;
        std::vector<uint64_t> starts(room), ends(room), groups(room * pairs * 2);
        uint64_t hits = 0;
        const int rc = bmx_search_regex_groups(nullptr, text.data(), n, &re, gr.get(), posix ? BMX_REGEX_LONGEST : 0u, starts.data(), ends.data(),
                                               groups.data(), room, &hits);
        if (rc != BMX_OK) {
            fprintf(stderr, "bmx_search_regex_groups failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        for (uint64_t i = 0; i < hits && i < max_print; ++i) {
            printf("%llu\t%llu", (unsigned long long)starts[i], (unsigned long long)ends[i]);
            for (uint64_t g = 1; g < pairs; ++g) {
                const uint64_t b = groups[(i * pairs + g) * 2], e = groups[(i * pairs + g) * 2 + 1];
                if (b == UINT64_MAX) printf("\t-");
                else printf("\t%llu,%llu", (unsigned long long)b, (unsigned long long)e);
            }
            printf("\n");
        }
        printf("matches with groups: %llu (%d groups, %d positions, %d..%d bytes)\n", (unsigned long long)hits, gr->n_groups, re.m, re.min_len,
               re.max_len);
        return 0;
    }
    if (lines_mode || subst_mode) {
        bmx_ctx *ctx = nullptr;
        int rc = bmx_ctx_create(device, &ctx);
        if (rc != BMX_OK) {
            fprintf(stderr, "no device %d: %d (%s)\n", device, rc, bmx_last_error());
            return 1;
        }
        std::vector<uint64_t> off(n + 1);
        uint64_t rows = 0, longest = 4096, hits = 0, len = 0;
        const uint32_t longest_flag = select_merge ? 1u : 0u; // BMX_GAPS_LONGEST == BMX_REGEX_LONGEST: the smallest start of every end
        static_assert(BMX_GAPS_LONGEST == 1u && BMX_REGEX_LONGEST == 1u, "one flag for both starts passes");
        if (!lines_mode) off.resize(1);
        rc = lines_mode ? bmx_rows_split(ctx, text.data(), n, '\n', off.data(), off.size(), &rows, &longest) : BMX_OK;
        if (rc != BMX_OK) {
            fprintf(stderr, "bmx_rows_split failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        // every match as (start, end): the searches that report ends with the starts of their default rule
        const uint64_t room = n ? n : 1;
        std::vector<uint64_t> starts(room), ends(room);
        std::vector<uint8_t> dist(approx_k >= 0 ? room : 1);
        const char *what = "bmx_search";
        bmx_regex re;
        std::unique_ptr<bmx_regex_groups> gr(new bmx_regex_groups); // (--regex-groups: beside re)
        if (have_regex) {
            bmx_regex_long rl; // (--regex-long: in place of re)
            bmx_regex_anchors an; // (full where the expression has no assertions: read by the anchored entries only)
            if ((regex_anchored ? bmx_compile_regex_anchored(regex_expr.data(), regex_expr.size(), class_flags | anchor_flags, &re, &an)
                 : regex_groups ? bmx_compile_regex_groups(regex_expr.data(), regex_expr.size(), class_flags, &re, gr.get())
                 : regex_long   ? bmx_compile_regex_long(regex_expr.data(), regex_expr.size(), class_flags, &rl)
                 : regex_star   ? bmx_compile_regex_star(regex_expr.data(), regex_expr.size(), class_flags, &re)
                                : bmx_compile_regex(regex_expr.data(), regex_expr.size(), class_flags, &re)) != BMX_OK) {
                fprintf(stderr, "bad regular expression %s (%s)\n", regex_expr.c_str(), bmx_last_error());
                return 1;
            }
            // (the star search: a match longer than the longest row lies in no row)
            const uint32_t window = (uint32_t)std::min<uint64_t>(BMX_MAX_REGEX_STAR_WINDOW, std::max<uint64_t>(longest, 1));
            what = regex_star ? "bmx_search_regex_star_spans" : regex_long ? "bmx_search_regex_long_spans" : "bmx_search_regex_spans";
            uint64_t clipped = 0; // --regex-star --posix: the starts whose longest match may be longer than the window
            if (posix && !lines_mode && regex_star) {
                what = "bmx_search_regex_star_begins_spans";
                rc = bmx_search_regex_star_begins_spans(ctx, text.data(), n, &re, star_window, BMX_REGEX_LONGEST, starts.data(), ends.data(), room,
                                                        &hits, &clipped);
            } else if (posix && !lines_mode) { // every start with its longest end: the selection below gives leftmost-longest
                what = "bmx_search_regex_begins_spans";
                rc = regex_anchored ? bmx_search_regex_anchored_begins_spans(ctx, text.data(), n, &re, &an, BMX_REGEX_LONGEST, starts.data(),
                                                                             ends.data(), room, &hits)
                                    : bmx_search_regex_begins_spans(ctx, text.data(), n, &re, BMX_REGEX_LONGEST, starts.data(), ends.data(), room, &hits);
            } else if (posix) { // ... its longest end inside its line: the ends pass with the line's last byte as the limit
                what = "bmx_search_regex_begins_device / bmx_regex_ends_device";
                void *d_text = nullptr, *d_limit = nullptr;
                uint64_t *d_starts = nullptr, *d_ends = nullptr;
                rc = bmx_text_upload(ctx, text.data(), n, &d_text);
                if (rc == BMX_OK) rc = bmx_device_alloc(ctx, room * sizeof(uint64_t), (void **)&d_starts);
                if (rc == BMX_OK) rc = bmx_device_alloc(ctx, room * sizeof(uint64_t), (void **)&d_ends);
                if (rc == BMX_OK)
                    rc = regex_anchored ? bmx_search_regex_anchored_begins_device(ctx, d_text, n, 0, 0, &re, &an, '\n', '\n', d_starts, room, &hits, nullptr)
                         : regex_star   ? bmx_search_regex_star_begins_device(ctx, d_text, n, 0, 0, &re, d_starts, room, &hits, nullptr)
                                        : bmx_search_regex_begins_device(ctx, d_text, n, 0, 0, &re, d_starts, room, &hits, nullptr);
                if (rc == BMX_OK) rc = bmx_device_download(ctx, starts.data(), d_starts, hits * sizeof(uint64_t));
                std::vector<uint64_t> limit(hits ? hits : 1);
                for (uint64_t i = 0; i < hits && rc == BMX_OK; ++i) // off[0] = 0 and off[rows] = n: every start lies in a row
                    limit[i] = *std::upper_bound(off.begin(), off.begin() + rows + 1, starts[i]) - 1;
                if (rc == BMX_OK) rc = bmx_text_upload(ctx, reinterpret_cast<const char *>(limit.data()), hits * sizeof(uint64_t), &d_limit);
                if (rc == BMX_OK)
                    rc = regex_anchored ? bmx_regex_anchored_ends_device(ctx, d_text, n, 0, &re, &an, '\n', '\n', d_starts, hits,
                                                                         static_cast<const uint64_t *>(d_limit), BMX_REGEX_LONGEST, d_ends, nullptr)
                         : regex_star ? bmx_regex_star_ends_device(ctx, d_text, n, 0, &re, d_starts, hits, static_cast<const uint64_t *>(d_limit),
                                                                 star_window, BMX_REGEX_LONGEST, d_ends, &clipped, nullptr)
                                    : bmx_regex_ends_device(ctx, d_text, n, 0, &re, d_starts, hits, static_cast<const uint64_t *>(d_limit),
                                                            BMX_REGEX_LONGEST, d_ends, nullptr);
                if (rc == BMX_OK) rc = bmx_device_download(ctx, ends.data(), d_ends, hits * sizeof(uint64_t));
                bmx_device_free(ctx, d_limit);
                bmx_device_free(ctx, d_ends);
                bmx_device_free(ctx, d_starts);
                bmx_device_free(ctx, d_text);
            } else
            rc = regex_anchored ? bmx_search_regex_anchored_spans(ctx, text.data(), n, &re, &an, longest_flag, starts.data(), ends.data(), room, &hits)
                 : regex_long ? bmx_search_regex_long_spans(ctx, text.data(), n, &rl, longest_flag, starts.data(), ends.data(), room, &hits)
                 : regex_star ? bmx_search_regex_star_spans(ctx, text.data(), n, &re, window, longest_flag, starts.data(), ends.data(), room, &hits)
                            : bmx_search_regex_spans(ctx, text.data(), n, &re, longest_flag, starts.data(), ends.data(), room, &hits);
            if (rc == BMX_OK && clipped != 0) { // never a shorter match than POSIX's
                fprintf(stderr, "--posix: %llu match(es) may be longer than the window of %u bytes; pass a larger --window\n",
                        (unsigned long long)clipped, star_window);
                return 1;
            }
        } else if (have_gaps) {
            what = "bmx_search_gaps_spans";
            rc = bmx_search_gaps_spans(ctx, text.data(), n, classes.data(), m, gaps_optional, longest_flag, starts.data(), ends.data(), room, &hits);
        } else if (approx_k >= 0) {
            what = "bmx_search_approx_spans";
            if (have_classes)
                rc = bmx_search_approx_spans_classes(ctx, text.data(), n, classes.data(), m, approx_k, 0, starts.data(), ends.data(),
                                                     dist.data(), room, &hits);
            else if (m > BMX_MAX_APPROX_PATTERN)
                rc = bmx_search_approx_long_spans(ctx, text.data(), n, pat.data(), m, approx_k, 0, starts.data(), ends.data(), dist.data(),
                                                  room, &hits);
            else
                rc = bmx_search_approx_spans(ctx, text.data(), n, pat.data(), m, approx_k, 0, starts.data(), ends.data(), dist.data(), room,
                                             &hits);
        } else if (have_classes) {
            what = "bmx_search_classes";
            len = (uint64_t)m;
            rc = bmx_search_classes(ctx, text.data(), n, classes.data(), m, starts.data(), room, &hits);
        } else {
            len = (uint64_t)m;
            rc = bmx_search(ctx, text.data(), n, pat.data(), m, starts.data(), room, &hits);
        }
        if (rc != BMX_OK) {
            fprintf(stderr, "%s failed: %d (%s)\n", what, rc, bmx_last_error());
            return 1;
        }
        std::vector<uint64_t> row(hits ? hits : 1), out(rows ? rows : 1), counts(rows ? rows : 1);
        uint64_t n_out = 0;
        if (subst_mode) {
            if (lines_mode && (rc = bmx_rows_of(ctx, off.data(), rows, starts.data(), len ? nullptr : ends.data(), len, hits, row.data())) != BMX_OK) {
                fprintf(stderr, "bmx_rows_of failed: %d (%s)\n", rc, bmx_last_error());
                return 1;
            }
            std::vector<uint64_t> sel_s(hits ? hits : 1), sel_e(hits ? hits : 1), blob_off(hits + 1);
            uint64_t taken = 0, n_new = 0;
            rc = bmx_spans_select(ctx, starts.data(), len ? nullptr : ends.data(), len, hits, lines_mode ? row.data() : nullptr,
                                  select_merge ? BMX_SELECT_MERGE : 0u, sel_s.data(), sel_e.data(), nullptr, hits, &taken);
            if (rc != BMX_OK) {
                fprintf(stderr, "bmx_spans_select failed: %d (%s)\n", rc, bmx_last_error());
                return 1;
            }
            std::string result(have_replace ? n + taken * replace_str.size() + 1 : n + 1, '\0');
            if (regex_groups) { // the groups of the matches taken, then the copy with the template: counted first, then filled
                const std::string &tmpl = have_replace ? replace_str : template_str;
                const uint64_t words = taken * ((uint64_t)gr->n_groups + 1) * 2;
                std::vector<uint64_t> groups(words ? words : 1);
                void *d_text = nullptr, *d_s = nullptr, *d_e = nullptr;
                uint64_t *d_groups = nullptr;
                what = "bmx_regex_groups_device";
                if (taken) {
                    rc = bmx_text_upload(ctx, text.data(), n, &d_text);
                    if (rc == BMX_OK) rc = bmx_text_upload(ctx, reinterpret_cast<const char *>(sel_s.data()), taken * sizeof(uint64_t), &d_s);
                    if (rc == BMX_OK) rc = bmx_text_upload(ctx, reinterpret_cast<const char *>(sel_e.data()), taken * sizeof(uint64_t), &d_e);
                    if (rc == BMX_OK) rc = bmx_device_alloc(ctx, words * sizeof(uint64_t), (void **)&d_groups);
                    if (rc == BMX_OK)
                        rc = bmx_regex_groups_device(ctx, d_text, n, 0, &re, gr.get(), static_cast<const uint64_t *>(d_s),
                                                     static_cast<const uint64_t *>(d_e), taken, d_groups, nullptr);
                    if (rc == BMX_OK) rc = bmx_device_download(ctx, groups.data(), d_groups, words * sizeof(uint64_t));
                    bmx_device_free(ctx, d_groups);
                    bmx_device_free(ctx, d_e);
                    bmx_device_free(ctx, d_s);
                    bmx_device_free(ctx, d_text);
                }
                const uint32_t flags = have_replace ? 0u : BMX_EXPAND_EXTRACT;
                if (rc == BMX_OK) {
                    what = "bmx_expand";
                    rc = bmx_expand(ctx, text.data(), n, groups.data(), gr->n_groups, taken, tmpl.data(), tmpl.size(), flags, nullptr, 0,
                                    blob_off.data(), &n_new);
                }
                if (rc == BMX_OK) {
                    result.assign(n_new + 1, '\0');
                    rc = bmx_expand(ctx, text.data(), n, groups.data(), gr->n_groups, taken, tmpl.data(), tmpl.size(), flags, &result[0],
                                    result.size(), blob_off.data(), &n_new);
                }
            } else {
                what = have_replace ? "bmx_replace" : "bmx_extract";
                rc = have_replace ? bmx_replace(ctx, text.data(), n, sel_s.data(), sel_e.data(), 0, taken, replace_str.data(), replace_str.size(),
                                                &result[0], result.size(), &n_new)
                                  : bmx_extract(ctx, text.data(), n, sel_s.data(), sel_e.data(), 0, taken, &result[0], result.size(),
                                                blob_off.data(), &n_new);
            }
            if (rc != BMX_OK) {
                fprintf(stderr, "%s failed: %d (%s)\n", what, rc, bmx_last_error());
                return 1;
            }
            FILE *dst = out_path.empty() ? stdout : fopen(out_path.c_str(), "wb");
            if (!dst) {
                fprintf(stderr, "cannot write %s\n", out_path.c_str());
                return 1;
            }
            if (have_replace) {
                fwrite(result.data(), 1, n_new, dst);
                fprintf(stderr, "replaced %llu of %llu matches: %llu bytes -> %llu bytes\n", (unsigned long long)taken, (unsigned long long)hits,
                        (unsigned long long)n, (unsigned long long)n_new);
            } else {
                for (uint64_t i = 0; i < taken && i < max_print; ++i) {
                    fwrite(result.data() + blob_off[i], 1, blob_off[i + 1] - blob_off[i], dst);
                    fputc('\n', dst);
                }
                fprintf(stderr, "matches: %llu of %llu taken (%llu bytes)\n", (unsigned long long)taken, (unsigned long long)hits,
                        (unsigned long long)n_new);
            }
            if (dst != stdout) fclose(dst);
            bmx_ctx_destroy(ctx);
            return 0;
        }
        rc = bmx_rows_of(ctx, off.data(), rows, starts.data(), len ? nullptr : ends.data(), len, hits, row.data());
        if (rc == BMX_OK)
            rc = bmx_rows_matching(ctx, row.data(), hits, rows, lines_invert ? BMX_ROWS_INVERT : 0u, out.data(),
                                   lines_invert ? nullptr : counts.data(), rows, &n_out);
        if (rc != BMX_OK) {
            fprintf(stderr, "bmx_rows_of / bmx_rows_matching failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        for (uint64_t i = 0; i < n_out && i < max_print; ++i) {
            if (lines_invert) printf("%llu\n", (unsigned long long)out[i]);
            else printf("%llu\t%llu\n", (unsigned long long)out[i], (unsigned long long)counts[i]);
        }
        printf("lines %s: %llu of %llu (%llu matches, longest line %llu bytes)\n", lines_invert ? "without a match" : "with a match",
               (unsigned long long)n_out, (unsigned long long)rows, (unsigned long long)hits, (unsigned long long)longest);
        bmx_ctx_destroy(ctx);
        return 0;
    }
    if (have_regex) {
        bmx_regex re;
        bmx_regex_long rl; // (--regex-long: in place of re)
        bmx_regex_anchors an; // (read by the anchored entries only)
        if ((regex_anchored ? bmx_compile_regex_anchored(regex_expr.data(), regex_expr.size(), class_flags | anchor_flags, &re, &an)
             : regex_long   ? bmx_compile_regex_long(regex_expr.data(), regex_expr.size(), class_flags, &rl)
             : regex_star   ? bmx_compile_regex_star(regex_expr.data(), regex_expr.size(), class_flags, &re)
                            : bmx_compile_regex(regex_expr.data(), regex_expr.size(), class_flags, &re)) != BMX_OK) {
            fprintf(stderr, "bad regular expression %s (%s)\n", regex_expr.c_str(), bmx_last_error());
            return 1;
        }
        if (regex_long) re.m = rl.m, re.min_len = rl.min_len, re.max_len = rl.max_len; // (for the line below)
        if (re.max_len == BMX_REGEX_UNBOUNDED)
            printf("text %s: %llu bytes, regular expression %s: %d positions, matches of %d or more bytes\n", text_path.c_str(),
                   (unsigned long long)n, regex_expr.c_str(), re.m, re.min_len);
        else
            printf("text %s: %llu bytes, regular expression %s: %d positions, matches of %d to %d bytes\n", text_path.c_str(),
                   (unsigned long long)n, regex_expr.c_str(), re.m, re.min_len, re.max_len);
        if (regex_begins) { // the starts (and an end of each) through the host-buffer entry points
            bmx_ctx *ctx = nullptr;
            int rc = bmx_ctx_create(device, &ctx);
            if (rc != BMX_OK) {
                fprintf(stderr, "no device %d: %d (%s)\n", device, rc, bmx_last_error());
                return 1;
            }
            const uint64_t room = n ? n : 1; // at most one hit per start
            std::vector<uint64_t> starts(room), ends(begins_spans ? room : 1);
            uint64_t got = 0, clipped = 0;
            const uint32_t span_flags = begins_longest ? BMX_REGEX_LONGEST : 0u;
            if (regex_anchored)
                rc = begins_spans ? bmx_search_regex_anchored_begins_spans(ctx, text.data(), n, &re, &an, span_flags, starts.data(), ends.data(), room, &got)
                                  : bmx_search_regex_anchored_begins(ctx, text.data(), n, &re, &an, starts.data(), room, &got);
            else if (regex_star)
                rc = begins_spans ? bmx_search_regex_star_begins_spans(ctx, text.data(), n, &re, star_window, span_flags, starts.data(), ends.data(),
                                                                       room, &got, &clipped)
                                  : bmx_search_regex_star_begins(ctx, text.data(), n, &re, starts.data(), room, &got);
            else
                rc = begins_spans ? bmx_search_regex_begins_spans(ctx, text.data(), n, &re, span_flags, starts.data(), ends.data(), room, &got)
                                  : bmx_search_regex_begins(ctx, text.data(), n, &re, starts.data(), room, &got);
            if (rc != BMX_OK) {
                fprintf(stderr, "bmx_search_regex%s_begins%s failed: %d (%s)\n", regex_star ? "_star" : "", begins_spans ? "_spans" : "", rc,
                        bmx_last_error());
                return 1;
            }
            printf("regex match starts: %llu\n", (unsigned long long)got);
            if (regex_star && begins_spans) printf("clipped by the window of %u bytes: %llu\n", star_window, (unsigned long long)clipped);
            if (got) {
                printf("first start: %llu\n", (unsigned long long)starts[0]);
                printf("last start: %llu\n", (unsigned long long)starts[got - 1]);
            }
            if (positions) {
                for (uint64_t i = 0; i < got && i < max_print; ++i) {
                    if (begins_spans) printf("Match at : %llu %llu\n", (unsigned long long)starts[i], (unsigned long long)ends[i]);
                    else printf("Start at : %llu\n", (unsigned long long)starts[i]);
                }
                if (got > max_print) printf("... %llu more\n", (unsigned long long)(got - max_print));
            }
            bmx_ctx_destroy(ctx);
            return 0;
        }
        bmx_ctx *ctx = nullptr;
        int rc = bmx_ctx_create(device, &ctx);
        void *d_text = nullptr;
        uint64_t *d_ends = nullptr;
        const uint64_t cap = n ? n : 1; // at most one hit per end
        if (rc == BMX_OK) rc = bmx_text_upload(ctx, text.data(), n, &d_text);
        if (rc == BMX_OK) rc = bmx_device_alloc(ctx, cap * sizeof(uint64_t), (void **)&d_ends);
        if (rc != BMX_OK) {
            fprintf(stderr, "device setup failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        double total = 0.0, kernel_ms = 0.0;
        uint64_t hits = 0;
        for (int it = 0; it < iters; ++it) {
            auto t0 = std::chrono::steady_clock::now();
            rc = regex_anchored ? bmx_search_regex_anchored_device(ctx, d_text, n, 0, 0, &re, &an, '\n', '\n', d_ends, cap, &hits, nullptr)
                 : regex_long ? bmx_search_regex_long_device(ctx, d_text, n, 0, 0, &rl, d_ends, cap, &hits, nullptr)
                 : regex_star ? bmx_search_regex_star_device(ctx, d_text, n, 0, 0, &re, d_ends, cap, &hits, nullptr)
                            : bmx_search_regex_device(ctx, d_text, n, 0, 0, &re, d_ends, cap, &hits, nullptr);
            auto t1 = std::chrono::steady_clock::now();
            if (rc != BMX_OK) {
                fprintf(stderr, "bmx_search_regex_device failed: %d (%s)\n", rc, bmx_last_error());
                return 1;
            }
            total += std::chrono::duration<double>(t1 - t0).count();
            kernel_ms += regex_anchored ? bmx_last_regex_anchored_ms(ctx) : regex_long ? bmx_last_regex_long_ms(ctx) : regex_star ? bmx_last_regex_star_ms(ctx) : bmx_last_regex_ms(ctx);
        }
        if (iters <= 0) { // no timed call has counted: a counting call
            rc = regex_anchored ? bmx_search_regex_anchored(ctx, text.data(), n, &re, &an, nullptr, 0, &hits)
                 : regex_long ? bmx_search_regex_long(ctx, text.data(), n, &rl, nullptr, 0, &hits)
                 : regex_star ? bmx_search_regex_star(ctx, text.data(), n, &re, nullptr, 0, &hits)
                            : bmx_search_regex(ctx, text.data(), n, &re, nullptr, 0, &hits);
            if (rc != BMX_OK && rc != BMX_ERR_CAPACITY) hits = 0;
        }
        // the list itself through the host-buffer entry points: (text, automaton) -> ends, or -> (starts, ends)
        std::vector<uint64_t> ends(hits ? hits : 1), starts(gaps_starts && hits ? hits : 1);
        uint64_t got = 0;
        const uint32_t span_flags = gaps_longest ? BMX_REGEX_LONGEST : 0u;
        if (regex_anchored)
            rc = gaps_starts ? bmx_search_regex_anchored_spans(ctx, text.data(), n, &re, &an, span_flags, starts.data(), ends.data(), hits, &got)
                             : bmx_search_regex_anchored(ctx, text.data(), n, &re, &an, ends.data(), hits, &got);
        else if (regex_long)
            rc = gaps_starts ? bmx_search_regex_long_spans(ctx, text.data(), n, &rl, span_flags, starts.data(), ends.data(), hits, &got)
                             : bmx_search_regex_long(ctx, text.data(), n, &rl, ends.data(), hits, &got);
        else if (regex_star)
            rc = gaps_starts ? bmx_search_regex_star_spans(ctx, text.data(), n, &re, star_window, span_flags, starts.data(), ends.data(),
                                                           hits, &got)
                             : bmx_search_regex_star(ctx, text.data(), n, &re, ends.data(), hits, &got);
        else
            rc = gaps_starts ? bmx_search_regex_spans(ctx, text.data(), n, &re, span_flags, starts.data(), ends.data(), hits, &got)
                             : bmx_search_regex(ctx, text.data(), n, &re, ends.data(), hits, &got);
        if (rc != BMX_OK || got != hits) {
            fprintf(stderr, "%s failed: %d (%s), %llu hits against %llu\n", gaps_starts ? "bmx_search_regex_spans" : "bmx_search_regex",
                    rc, bmx_last_error(), (unsigned long long)got, (unsigned long long)hits);
            return 1;
        }
        printf("regex matches: %llu\n", (unsigned long long)got);
        if (got) {
            printf("first end: %llu\n", (unsigned long long)ends[0]);
            printf("last end: %llu\n", (unsigned long long)ends[got - 1]);
        }
        if (positions) {
            for (uint64_t i = 0; i < got && i < max_print; ++i) {
                if (gaps_starts) printf("Match at : %llu %llu\n", (unsigned long long)starts[i], (unsigned long long)ends[i]);
                else printf("End at : %llu\n", (unsigned long long)ends[i]);
            }
            if (got > max_print) printf("... %llu more\n", (unsigned long long)(got - max_print));
        }
        if (iters > 0)
            printf("Average time = %.6f s  (kernel %.3f ms)\n", total / iters, kernel_ms / iters);
        bmx_device_free(ctx, d_ends);
        bmx_device_free(ctx, d_text);
        bmx_ctx_destroy(ctx);
        return 0;
    }
    if (have_gaps)
        printf("text %s: %llu bytes, gapped pattern %s: %d positions, %d of them optional\n", text_path.c_str(),
               (unsigned long long)n, gaps_expr.c_str(), m, __builtin_popcountll(gaps_optional));
    else if (have_classes)
        printf("text %s: %llu bytes, class expression %s: %d positions\n", text_path.c_str(), (unsigned long long)n,
               class_expr.c_str(), m);
    else if (dict_path.empty())
        printf("text %s: %llu bytes, pattern %s: %d bytes\n", text_path.c_str(), (unsigned long long)n,
               pat_path.c_str(), m);
    else
        printf("text %s: %llu bytes\n", text_path.c_str(), (unsigned long long)n);

    if (!dict_path.empty()) {
        std::string words;
        if (!read_file(dict_path, words)) {
            fprintf(stderr, "File Not Found!\n");
            return 1;
        }
        std::vector<std::string> list;
        for (size_t at = 0; at < words.size();) {
            size_t nl = words.find('\n', at);
            if (nl == std::string::npos) nl = words.size();
            std::string w = words.substr(at, nl - at);
            if (!w.empty() && w.back() == '\r') w.pop_back();
            if (!w.empty()) list.push_back(w);
            at = nl + 1;
        }
        std::vector<const char *> pats;
        std::vector<int32_t> ms;
        for (const auto &w : list) pats.push_back(w.data()), ms.push_back((int32_t)w.size());
        const int32_t K = (int32_t)list.size();
        printf("dictionary %s: %d patterns\n", dict_path.c_str(), K);
        bmx_ctx *ctx = nullptr;
        bmx_dict *dict = nullptr;
        void *d_text = nullptr;
        int rc = bmx_ctx_create(device, &ctx);
        if (rc == BMX_OK) rc = bmx_dict_create(ctx, pats.data(), ms.data(), K, &dict);
        if (rc == BMX_OK && n) rc = bmx_text_upload(ctx, text.data(), n, &d_text);
        if (rc != BMX_OK) {
            fprintf(stderr, "device setup failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        double total = 0.0, kernel_ms = 0.0;
        uint64_t hits = 0;
        for (int it = 0; it < iters; ++it) { // count only: the timed calls store nothing
            auto t0 = std::chrono::steady_clock::now();
            rc = bmx_dict_search_device(ctx, dict, d_text, n, n, 0, nullptr, nullptr, 0, &hits, nullptr);
            auto t1 = std::chrono::steady_clock::now();
            if (rc != BMX_OK && rc != BMX_ERR_CAPACITY) {
                fprintf(stderr, "bmx_dict_search_device failed: %d (%s)\n", rc, bmx_last_error());
                return 1;
            }
            total += std::chrono::duration<double>(t1 - t0).count();
            kernel_ms += bmx_last_dict_ms(ctx);
        }
        // the list itself through the host-buffer entry point (text, patterns) -> (positions, pattern indices)
        uint64_t got = 0;
        rc = bmx_dict_search(ctx, text.data(), n, pats.data(), ms.data(), K, nullptr, nullptr, 0, &got);
        if (rc != BMX_OK && rc != BMX_ERR_CAPACITY) {
            fprintf(stderr, "bmx_dict_search failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        std::vector<uint64_t> pos(got ? got : 1);
        std::vector<uint32_t> pid(got ? got : 1);
        uint64_t got2 = 0;
        rc = bmx_dict_search(ctx, text.data(), n, pats.data(), ms.data(), K, pos.data(), pid.data(), got, &got2);
        if (rc != BMX_OK || got2 != got || (iters > 0 && got != hits)) {
            fprintf(stderr, "bmx_dict_search failed: %d (%s), %llu pairs against %llu\n", rc, bmx_last_error(),
                    (unsigned long long)got2, (unsigned long long)got);
            return 1;
        }
        printf("dictionary matches: %llu\n", (unsigned long long)got);
        if (got) {
            printf("first match: %llu (pattern %u)\n", (unsigned long long)pos[0], pid[0]);
            printf("last match: %llu (pattern %u)\n", (unsigned long long)pos[got - 1], pid[got - 1]);
        }
        if (positions) {
            for (uint64_t i = 0; i < got && i < max_print; ++i)
                printf("Match at : %llu (pattern %u)\n", (unsigned long long)pos[i], pid[i]);
            if (got > max_print) printf("... %llu more\n", (unsigned long long)(got - max_print));
        }
        if (iters > 0)
            printf("Average time = %.6f s  (kernel %.3f ms)\n", total / iters, kernel_ms / iters);
        if (d_text) bmx_device_free(ctx, d_text);
        bmx_dict_destroy(dict);
        bmx_ctx_destroy(ctx);
        return 0;
    }

    if (have_gaps) {
        bmx_ctx *ctx = nullptr;
        int rc = bmx_ctx_create(device, &ctx);
        void *d_text = nullptr;
        uint64_t *d_ends = nullptr;
        const uint64_t cap = n ? n : 1; // at most one hit per end
        if (rc == BMX_OK) rc = bmx_text_upload(ctx, text.data(), n, &d_text);
        if (rc == BMX_OK) rc = bmx_device_alloc(ctx, cap * sizeof(uint64_t), (void **)&d_ends);
        if (rc != BMX_OK) {
            fprintf(stderr, "device setup failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        double total = 0.0, kernel_ms = 0.0;
        uint64_t hits = 0;
        for (int it = 0; it < iters; ++it) {
            auto t0 = std::chrono::steady_clock::now();
            rc = bmx_search_gaps_device(ctx, d_text, n, 0, 0, classes.data(), m, gaps_optional, d_ends, cap, &hits, nullptr);
            auto t1 = std::chrono::steady_clock::now();
            if (rc != BMX_OK) {
                fprintf(stderr, "bmx_search_gaps_device failed: %d (%s)\n", rc, bmx_last_error());
                return 1;
            }
            total += std::chrono::duration<double>(t1 - t0).count();
            kernel_ms += bmx_last_gaps_ms(ctx);
        }
        if (iters <= 0) { // no timed call has counted: a counting call
            rc = bmx_search_gaps(ctx, text.data(), n, classes.data(), m, gaps_optional, nullptr, 0, &hits);
            if (rc != BMX_OK && rc != BMX_ERR_CAPACITY) hits = 0;
        }
        // the list itself through the host-buffer entry points: (text, pattern) -> ends, or -> (starts, ends)
        std::vector<uint64_t> ends(hits ? hits : 1), starts(gaps_starts && hits ? hits : 1);
        uint64_t got = 0;
        rc = gaps_starts ? bmx_search_gaps_spans(ctx, text.data(), n, classes.data(), m, gaps_optional,
                                                 gaps_longest ? BMX_GAPS_LONGEST : 0u, starts.data(), ends.data(), hits, &got)
                         : bmx_search_gaps(ctx, text.data(), n, classes.data(), m, gaps_optional, ends.data(), hits, &got);
        if (rc != BMX_OK || got != hits) {
            fprintf(stderr, "%s failed: %d (%s), %llu hits against %llu\n", gaps_starts ? "bmx_search_gaps_spans" : "bmx_search_gaps",
                    rc, bmx_last_error(), (unsigned long long)got, (unsigned long long)hits);
            return 1;
        }
        printf("gapped matches: %llu\n", (unsigned long long)got);
        if (got) {
            printf("first end: %llu\n", (unsigned long long)ends[0]);
            printf("last end: %llu\n", (unsigned long long)ends[got - 1]);
        }
        if (positions) {
            for (uint64_t i = 0; i < got && i < max_print; ++i) {
                if (gaps_starts) printf("Match at : %llu %llu\n", (unsigned long long)starts[i], (unsigned long long)ends[i]);
                else printf("End at : %llu\n", (unsigned long long)ends[i]);
            }
            if (got > max_print) printf("... %llu more\n", (unsigned long long)(got - max_print));
        }
        if (iters > 0)
            printf("Average time = %.6f s  (kernel %.3f ms)\n", total / iters, kernel_ms / iters);
        bmx_device_free(ctx, d_ends);
        bmx_device_free(ctx, d_text);
        bmx_ctx_destroy(ctx);
        return 0;
    }

    if (hamming_k >= 0) {
        bmx_ctx *ctx = nullptr;
        int rc = bmx_ctx_create(device, &ctx);
        void *d_text = nullptr;
        uint64_t *d_starts = nullptr;
        uint8_t *d_dist = nullptr;
        const uint64_t cap = n ? n : 1; // at most one hit per start
        if (rc == BMX_OK) rc = bmx_text_upload(ctx, text.data(), n, &d_text);
        if (rc == BMX_OK) rc = bmx_device_alloc(ctx, cap * sizeof(uint64_t), (void **)&d_starts);
        if (rc == BMX_OK) rc = bmx_device_alloc(ctx, cap, (void **)&d_dist);
        if (rc != BMX_OK) {
            fprintf(stderr, "device setup failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        double total = 0.0, kernel_ms = 0.0;
        uint64_t hits = 0;
        for (int it = 0; it < iters; ++it) {
            auto t0 = std::chrono::steady_clock::now();
            rc = have_classes ? bmx_search_hamming_classes_device(ctx, d_text, n, n, 0, classes.data(), m, hamming_k, must, d_starts,
                                                                  d_dist, cap, &hits, nullptr)
                              : bmx_search_hamming_device(ctx, d_text, n, n, 0, pat.data(), m, hamming_k, must, d_starts, d_dist, cap,
                                                          &hits, nullptr);
            auto t1 = std::chrono::steady_clock::now();
            if (rc != BMX_OK) {
                fprintf(stderr, "%s failed: %d (%s)\n", have_classes ? "bmx_search_hamming_classes_device" : "bmx_search_hamming_device",
                        rc, bmx_last_error());
                return 1;
            }
            total += std::chrono::duration<double>(t1 - t0).count();
            kernel_ms += bmx_last_hamming_ms(ctx);
        }
        // the list itself through the host-buffer entry point (text, pattern, k, must) -> (starts, distances)
        std::vector<uint64_t> starts(hits ? hits : 1);
        std::vector<uint8_t> dist(hits ? hits : 1);
        uint64_t got = 0;
        if (have_classes)
            rc = bmx_search_hamming_classes(ctx, text.data(), n, classes.data(), m, hamming_k, must, starts.data(), dist.data(), hits,
                                            &got);
        else
            rc = bmx_search_hamming(ctx, text.data(), n, pat.data(), m, hamming_k, must, starts.data(), dist.data(), hits, &got);
        if (rc != BMX_OK || got != hits) {
            fprintf(stderr, "%s failed: %d (%s), %llu hits against %llu\n", have_classes ? "bmx_search_hamming_classes" : "bmx_search_hamming",
                    rc, bmx_last_error(), (unsigned long long)got, (unsigned long long)hits);
            return 1;
        }
        printf("k-mismatch matches (k = %d): %llu\n", hamming_k, (unsigned long long)hits);
        if (hits) {
            printf("first start: %llu (distance %d)\n", (unsigned long long)starts[0], dist[0]);
            printf("last start: %llu (distance %d)\n", (unsigned long long)starts[hits - 1], dist[hits - 1]);
        }
        if (positions) {
            for (uint64_t i = 0; i < hits && i < max_print; ++i)
                printf("Start at : %llu (distance %d)\n", (unsigned long long)starts[i], dist[i]);
            if (hits > max_print) printf("... %llu more\n", (unsigned long long)(hits - max_print));
        }
        if (iters > 0)
            printf("Average time = %.6f s  (kernel %.3f ms)\n", total / iters, kernel_ms / iters);
        bmx_device_free(ctx, d_dist);
        bmx_device_free(ctx, d_starts);
        bmx_device_free(ctx, d_text);
        bmx_ctx_destroy(ctx);
        return 0;
    }

    if (have_classes && approx_k < 0) {
        bmx_ctx *ctx = nullptr;
        int rc = bmx_ctx_create(device, &ctx);
        void *d_text = nullptr;
        uint64_t *d_starts = nullptr;
        const uint64_t cap = n ? n : 1; // at most one hit per start
        if (rc == BMX_OK) rc = bmx_text_upload(ctx, text.data(), n, &d_text);
        if (rc == BMX_OK) rc = bmx_device_alloc(ctx, cap * sizeof(uint64_t), (void **)&d_starts);
        if (rc != BMX_OK) {
            fprintf(stderr, "device setup failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        double total = 0.0, kernel_ms = 0.0;
        uint64_t hits = 0;
        for (int it = 0; it < iters; ++it) {
            auto t0 = std::chrono::steady_clock::now();
            rc = bmx_search_classes_device(ctx, d_text, n, n, 0, classes.data(), m, d_starts, cap, &hits, nullptr);
            auto t1 = std::chrono::steady_clock::now();
            if (rc != BMX_OK) {
                fprintf(stderr, "bmx_search_classes_device failed: %d (%s)\n", rc, bmx_last_error());
                return 1;
            }
            total += std::chrono::duration<double>(t1 - t0).count();
            kernel_ms += bmx_last_classes_ms(ctx);
        }
        // the list itself through the host-buffer entry point (text, classes) -> starts
        std::vector<uint64_t> starts(hits ? hits : 1);
        uint64_t got = 0;
        rc = bmx_search_classes(ctx, text.data(), n, classes.data(), m, starts.data(), hits, &got);
        if (rc != BMX_OK || got != hits) {
            fprintf(stderr, "bmx_search_classes failed: %d (%s), %llu hits against %llu\n", rc, bmx_last_error(),
                    (unsigned long long)got, (unsigned long long)hits);
            return 1;
        }
        printf("class matches: %llu\n", (unsigned long long)got);
        if (got) {
            printf("first start: %llu\n", (unsigned long long)starts[0]);
            printf("last start: %llu\n", (unsigned long long)starts[got - 1]);
        }
        if (positions) {
            for (uint64_t i = 0; i < got && i < max_print; ++i) printf("Start at : %llu\n", (unsigned long long)starts[i]);
            if (got > max_print) printf("... %llu more\n", (unsigned long long)(got - max_print));
        }
        if (iters > 0)
            printf("Average time = %.6f s  (kernel %.3f ms)\n", total / iters, kernel_ms / iters);
        bmx_device_free(ctx, d_starts);
        bmx_device_free(ctx, d_text);
        bmx_ctx_destroy(ctx);
        return 0;
    }

    if (approx_k >= 0) {
        bmx_ctx *ctx = nullptr;
        int rc = bmx_ctx_create(device, &ctx);
        void *d_text = nullptr;
        uint64_t *d_ends = nullptr;
        uint8_t *d_dist = nullptr;
        const uint64_t cap = n ? n : 1; // at most one hit per end
        if (rc == BMX_OK) rc = bmx_text_upload(ctx, text.data(), n, &d_text);
        if (rc == BMX_OK) rc = bmx_device_alloc(ctx, cap * sizeof(uint64_t), (void **)&d_ends);
        if (rc == BMX_OK) rc = bmx_device_alloc(ctx, cap, (void **)&d_dist);
        if (rc != BMX_OK) {
            fprintf(stderr, "device setup failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        double total = 0.0, kernel_ms = 0.0;
        uint64_t hits = 0;
        for (int it = 0; it < iters; ++it) {
            auto t0 = std::chrono::steady_clock::now();
            rc = have_classes ? bmx_search_approx_classes_device(ctx, d_text, n, 0, 0, classes.data(), m, approx_k, d_ends, d_dist,
                                                                 cap, &hits, nullptr)
                              : bmx_search_approx_long_device(ctx, d_text, n, 0, 0, pat.data(), m, approx_k, d_ends, d_dist, cap,
                                                              &hits, nullptr); // (any m up to 512; up to 64: the short entry's list)
            auto t1 = std::chrono::steady_clock::now();
            if (rc != BMX_OK) {
                fprintf(stderr, "%s failed: %d (%s)\n", have_classes ? "bmx_search_approx_classes_device" : "bmx_search_approx_long_device",
                        rc, bmx_last_error());
                return 1;
            }
            total += std::chrono::duration<double>(t1 - t0).count();
            kernel_ms += bmx_last_approx_ms(ctx);
        }
        // the list itself through the host-buffer entry point (text, pattern, k) -> (ends, distances)
        std::vector<uint64_t> ends(hits ? hits : 1);
        std::vector<uint8_t> dist(hits ? hits : 1);
        uint64_t got = 0;
        if (have_classes)
            rc = bmx_search_approx_classes(ctx, text.data(), n, classes.data(), m, approx_k, ends.data(), dist.data(), hits, &got);
        else
            rc = bmx_search_approx_long(ctx, text.data(), n, pat.data(), m, approx_k, ends.data(), dist.data(), hits, &got);
        if (rc != BMX_OK || got != hits) {
            fprintf(stderr, "%s failed: %d (%s), %llu hits against %llu\n",
                    have_classes ? "bmx_search_approx_classes" : "bmx_search_approx_long", rc, bmx_last_error(),
                    (unsigned long long)got, (unsigned long long)hits);
            return 1;
        }
        printf("approximate matches (k = %d): %llu\n", approx_k, (unsigned long long)hits);
        if (hits) {
            printf("first end: %llu (distance %d)\n", (unsigned long long)ends[0], dist[0]);
            printf("last end: %llu (distance %d)\n", (unsigned long long)ends[hits - 1], dist[hits - 1]);
        }
        if (positions) {
            for (uint64_t i = 0; i < hits && i < max_print; ++i)
                printf("End at : %llu (distance %d)\n", (unsigned long long)ends[i], dist[i]);
            if (hits > max_print) printf("... %llu more\n", (unsigned long long)(hits - max_print));
        }
        if (iters > 0)
            printf("Average time = %.6f s  (kernel %.3f ms)\n", total / iters, kernel_ms / iters);
        if (spans) { // (text, pattern, k) -> (starts, ends, distances) through the host-buffer entry point
            const uint32_t flags = spans_best ? BMX_SPANS_BEST : 0u;
            const uint64_t room = hits ? hits : 1; // never more spans than ends
            std::vector<uint64_t> s_starts(room), s_ends(room);
            std::vector<uint8_t> s_dist(room);
            uint64_t n_spans = 0;
            if (have_classes)
                rc = bmx_search_approx_spans_classes(ctx, text.data(), n, classes.data(), m, approx_k, flags, s_starts.data(),
                                                     s_ends.data(), s_dist.data(), room, &n_spans);
            else
                rc = bmx_search_approx_long_spans(ctx, text.data(), n, pat.data(), m, approx_k, flags, s_starts.data(), s_ends.data(),
                                                  s_dist.data(), room, &n_spans);
            if (rc != BMX_OK) {
                fprintf(stderr, "%s failed: %d (%s)\n", have_classes ? "bmx_search_approx_spans_classes" : "bmx_search_approx_long_spans",
                        rc, bmx_last_error());
                return 1;
            }
            printf("match spans%s: %llu  (spans kernels %.3f ms)\n", spans_best ? " (best)" : "", (unsigned long long)n_spans,
                   n_spans ? bmx_last_spans_ms(ctx) : 0.0);
            std::vector<std::string> scripts;
            if (cigar) {
                const uint64_t one_off[2] = {0, (uint64_t)m};
                s_starts.resize(n_spans), s_ends.resize(n_spans);
                if (!cigar_strings(ctx, text, 0, pat.data(), (uint64_t)m, one_off, 1, s_starts, s_ends, approx_k, scripts)) return 1;
            }
            for (uint64_t i = 0; i < n_spans && i < max_print; ++i) {
                printf("%llu %llu %d", (unsigned long long)s_starts[i], (unsigned long long)s_ends[i], s_dist[i]);
                if (cigar) printf(" %s", scripts[i].c_str());
                printf("\n");
            }
            if (n_spans > max_print) printf("... %llu more\n", (unsigned long long)(n_spans - max_print));
        }
        bmx_device_free(ctx, d_dist);
        bmx_device_free(ctx, d_ends);
        bmx_device_free(ctx, d_text);
        bmx_ctx_destroy(ctx);
        return 0;
    }

    int32_t bad[BMX_BAD_TABLE_SIZE];
    std::vector<int32_t> good(m > 0 ? m : 1);
    int rc = bmx_build_tables(pat.data(), m, bad, good.data());
    if (rc != BMX_OK) {
        fprintf(stderr, "bmx_build_tables failed: %d\n", rc);
        return 1;
    }

    bmx_ctx *ctx = nullptr;
    rc = bmx_ctx_create(device, &ctx);
    if (rc != BMX_OK) {
        fprintf(stderr, "bmx_ctx_create failed: %d (%s)\n", rc, bmx_last_error());
        return 1;
    }

    if (ranges > 0) {
        std::vector<int32_t> se = split_like_reference(text, ranges);
        std::vector<int32_t> ans(ranges);
        rc = bmx_search_ranges(ctx, text.data(), n, pat.data(), se.data(), ranges, ans.data(), good.data(), bad, m);
        if (rc != BMX_OK) {
            fprintf(stderr, "bmx_search_ranges failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        for (int r = 0; r < ranges; ++r)
            printf("The no. of occurrences by process %d is %d   [range %d..%d]\n", r, ans[r], se[2 * r], se[2 * r + 1]);
    }

    // text resident once, searched `iters` times (the reference's timer also
    // starts after the upload)
    void *d_text = nullptr;
    uint64_t *d_out = nullptr;
    const uint64_t cap = n >= (uint64_t)m ? n - (uint64_t)m + 1 : 1;
    rc = bmx_text_upload(ctx, text.data(), n, &d_text);
    if (rc == BMX_OK) rc = bmx_device_alloc(ctx, cap * sizeof(uint64_t), (void **)&d_out);
    if (rc != BMX_OK) {
        fprintf(stderr, "device setup failed: %d (%s)\n", rc, bmx_last_error());
        return 1;
    }
    double total = 0.0;
    uint64_t n_matches = 0;
    for (int it = 0; it < iters; ++it) {
        auto t0 = std::chrono::steady_clock::now();
        rc = bmx_search_device(ctx, d_text, n, n, 0, pat.data(), m, good.data(), bad, d_out, cap, &n_matches, nullptr);
        auto t1 = std::chrono::steady_clock::now();
        if (rc != BMX_OK) {
            fprintf(stderr, "bmx_search_device failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        const double s = std::chrono::duration<double>(t1 - t0).count();
        total += s;
        printf("Time Spent: %.6f s (scan kernel %.3f ms)\n", s, bmx_last_scan_ms(ctx));
    }
    printf("occurrences: %llu\n", (unsigned long long)n_matches);
    if (iters > 0) {
        const double avg = total / iters;
        printf("Average time = %.6f s  (%.3f GB/s)\n", avg, avg > 0 ? (double)n / avg / 1e9 : 0.0);
    }

    if (gpus > 0) {
        // The same search from this ONE host process over `gpus` devices (the reference drives all of its work-items from
        // one main, BoyreMoore.cpp:273-286): devices, RCCL communicators and the text are set up once (bmx_multi_*), then
        // `iters` searches run on the resident shards, each ending with one all-gather of match-offset slots.
        std::vector<uint64_t> one(n_matches ? n_matches : 1), many(n_matches ? n_matches : 1);
        uint64_t got1 = 0, gotN = 0;
        rc = bmx_search(ctx, text.data(), n, pat.data(), m, one.data(), one.size(), &got1);
        if (rc != BMX_OK) {
            fprintf(stderr, "bmx_search failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        bmx_multi *mg = nullptr;
        rc = bmx_multi_create(nullptr, gpus, &mg);
        if (rc == BMX_OK) rc = bmx_multi_text_upload(mg, text.data(), n, m);
        if (rc != BMX_OK) {
            fprintf(stderr, "bmx_multi over %d GPUs: set-up failed: %d (%s)\n", gpus, rc, bmx_last_error());
            return 1;
        }
        double total_multi = 0.0;
        for (int it = 0; it < iters; ++it) {
            auto t0 = std::chrono::steady_clock::now();
            rc = bmx_multi_search(mg, pat.data(), m, many.data(), many.size(), &gotN);
            auto t1 = std::chrono::steady_clock::now();
            if (rc != BMX_OK) {
                fprintf(stderr, "bmx_multi_search over %d GPUs failed: %d (%s)\n", gpus, rc, bmx_last_error());
                return 1;
            }
            total_multi += std::chrono::duration<double>(t1 - t0).count();
        }
        const char *how[] = {"none", "RCCL all-gather of slots", "slots staged through host memory", "exact path (dense result)"};
        bool same = got1 == gotN && std::equal(one.begin(), one.begin() + got1, many.begin());
        printf("%d GPUs, resident shards: %llu occurrences, average time = %.6f s (slowest scan kernel %.3f ms, exchange: %s), list %s the one-GPU list\n",
               gpus, (unsigned long long)gotN, iters > 0 ? total_multi / iters : 0.0, bmx_multi_last_scan_ms(mg),
               how[bmx_multi_last_exchange(mg) & 3], same ? "identical to" : "DIFFERS from");
        bmx_multi_destroy(mg);
        if (!same) return 1;
        // ... and through the host-buffer entry point (upload + search + download per call)
        auto t0 = std::chrono::steady_clock::now();
        rc = bmx_search_multi(text.data(), n, pat.data(), m, nullptr, gpus, many.data(), many.size(), &gotN);
        auto t1 = std::chrono::steady_clock::now();
        if (rc != BMX_OK) {
            fprintf(stderr, "bmx_search_multi over %d GPUs failed: %d (%s)\n", gpus, rc, bmx_last_error());
            return 1;
        }
        same = got1 == gotN && std::equal(one.begin(), one.begin() + got1, many.begin());
        printf("%d GPUs, host buffers in and out: %llu occurrences in %.6f s, list %s the one-GPU list\n", gpus,
               (unsigned long long)gotN, std::chrono::duration<double>(t1 - t0).count(),
               same ? "identical to" : "DIFFERS from");
        if (!same) return 1;
    }

    // the positions, through the host-buffer entry point (text, pattern, match_positions)
    if (positions) {
        std::vector<uint64_t> pos(n_matches ? n_matches : 1);
        uint64_t got = 0;
        rc = bmx_search(ctx, text.data(), n, pat.data(), m, pos.data(), pos.size(), &got);
        if (rc != BMX_OK) {
            fprintf(stderr, "bmx_search failed: %d (%s)\n", rc, bmx_last_error());
            return 1;
        }
        for (uint64_t i = 0; i < got && i < max_print; ++i) printf("Found at : %llu\n", (unsigned long long)pos[i]);
        if (got > max_print) printf("... %llu more\n", (unsigned long long)(got - max_print));
    }
    bmx_device_free(ctx, d_out);
    bmx_device_free(ctx, d_text);
    bmx_ctx_destroy(ctx);
    return 0;
}
