// hs_motif_search.cpp -- the `motif_both_points` program of the reference on the GPU path.
//
// Keeps the reference's command line (hclust/src/hclust/motif_both_points.cpp:302-320):
//     -d <db.points> -c <centers.points> -l <k> -W <w> -T <R> -g <groundtruth> -o <out>
// each also as -db/-center/-len/-window/-threshold/-groundtruth/-output (one or two dashes), and its
// exit behaviour: a missing required option prints the help text and exits 0 (:332-335), a runtime
// error prints to stderr and exits 1 (:387-393).  Additions: -K/-L (the reference parses them in
// kmer_search.cpp:186-189 but hard-codes 4,4 here, :380-381 -- 4,4 stay the defaults), --seed
// (planes are drawn like the reference's LSH constructor but from an explicit seed; default: from
// std::random_device like the reference), --planes <file> (read them instead: the binary doubles
// --planes-out writes), --device, --gpus n (the centres are sharded over GPUs
// device .. device+n-1 of this node, one host thread and one replicated index per GPU, hits
// all-gathered over RCCL and written in the same order -- the output file is the same for every
// n; --transport loopback runs the same rank threads with all ranks on --device and the exchange
// through host memory), and -g becomes optional (without it the evaluation step is skipped).  -c may also name a
// k-mer FASTA file (">name" + k letters, the format hclust2.cpp:231-241 reads): the centres are
// then embedded exactly from the table.  -d may also name a protein FASTA file (the
// database kmer_search.cpp:180-181 takes): every length-k window of every sequence is then a DB
// k-mer, enumerated on the device; --ref-compat-eq-swap reproduces the reference's E <-> Q exchange
// on that path.  --radii <file> (lines "<centre name> <radius>", any order, matched by name against the
// centres): every centre is searched at its own radius (hs_query_radii); -T is then not needed, and ignored
// with a notice if given; one GPU only.  --best-per-position 1: instead of the hits, one line per database k-mer
// reached, "<kmer name> <centre> <dist>" with its nearest centre (hs_annotate), k-mers ascending.  --topk N (1..64):
// per centre only its N best hits, selected on the device (hs_query_topk): the usual lines, per centre at most N of
// them, in ascending (distance, k-mer index); with points and FASTA databases, with --radii and -M; one GPU only, and
// not with --best-per-position 1.  --per-sequence 1 (FASTA database): instead of the hits, one line per (centre,
// protein) with a hit -- "<centre> <protein>#<number> <hits> <best window's offset> <its distance> <first> <last matched
// offset>" --, reduced on the device (hs_seq_match).  --query-fasta FILE in place of -c: the query proteins are cut
// into windows with the database's residue mapping and swap option, the groups are the query proteins and the lines
// are per (query protein, protein, diagonal), the diagonal last.  Both work with --radii (per centre, or per query
// protein) and -M; one GPU only, and not with --topk or --best-per-position 1.
// --pssm FILE (FASTA database): no search at all -- every window of every protein scored against the position-
// specific score matrices of FILE (hs_pssm_scan), one line per hit "<profile> <window name> <score>", the score with
// 17 significant digits; -c, -W and -T are not needed, and -c, --radii, -M, --topk, --per-sequence,
// --best-per-position, --query-fasta, --db-append and --gpus above 1 are refused.  With --pssm-top N (1..64): per
// profile at most N lines, its N best windows among those at or above the file's threshold (hs_pssm_topk), by
// descending score, then ascending window index; --pssm-top without --pssm is refused.  With --pssm-per-sequence 1:
// instead of the hits, one line per (profile, protein) with a hit -- "<profile> <protein>#<number> <hits> <best
// window's offset> <its score> <first> <last matched offset>" --, reduced on the device (hs_pssm_seq_scan), profiles in
// file order, proteins in database order; refused without --pssm and with --pssm-top.
// --pssm FILE --pssm-refine N --pssm-out FILE2 (N = 1..100): the profiles are first rebuilt from their own hits
// (hs_pssm_refine: scan, counts, log-odds against the database's residue composition with --pssm-pseudo x [1] pseudo-
// counts, at most N scans at the file's thresholds; --pssm-one-per-protein 1: only a protein's best window counts),
// written to FILE2 with their names and thresholds, and -o then holds exactly what a run with --pssm FILE2 writes
// (--pssm-top and --pssm-per-sequence included).  --pssm-refine without --pssm or without --pssm-out is refused.
// --pssm FILE --pssm-rank N --pssm-out FILE2: every threshold of FILE is replaced by the score of the profile's N-th
// best window over the database (hs_pssm_rank; N = 1 .. the number of windows), FILE2 is FILE with those thresholds,
// and -o holds exactly what --pssm FILE2 writes.  With --pssm-refine I beside it the loop scans at that threshold in
// every iteration (hs_pssm_refine_rank) and FILE2 holds the final matrices and the last scan's thresholds.
// --pssm-rank without --pssm or without --pssm-out is refused.
// --pssm-weights sites|columns beside --pssm-refine N (with or without --pssm-rank and --pssm-one-per-protein): the loop
// weighs its sites with position-based sequence weights (hs_pssm_refine_weighted) and takes the log-odds at n_eff = the
// sites or = the mean number of distinct residues per column; FILE2 and -o are written as --pssm-refine writes them.
// --pssm-weights without --pssm-refine, and any other value, are refused.
// --pssm FILE --pssm-pvalue P --pssm-out FILE2: every threshold of FILE is replaced by the threshold of the p-value P
// (0 < P <= 1) under the null model of the database's residue composition (hs_pssm_pvalue_threshold), on a score grid
// from --pssm-null-floor X [0] to the profile's maximal score; FILE2 is FILE with those thresholds and -o holds exactly
// what --pssm FILE2 writes (--pssm-top and --pssm-per-sequence included).  A profile on whose grid nothing is admissible
// keeps +DBL_MAX and finds nothing; it and the profiles clipped at the floor are reported on stderr by name.  Refused:
// --pssm-pvalue without --pssm or --pssm-out, with --pssm-rank or --pssm-refine, and a P that is no number in (0, 1].
// --pssm FILE --pssm-compare FILE2|self --pssm-compare-threshold T [--pssm-compare-overlap V] [--pssm-compare-columns
// pearson|cosine|raw]: no database at all (-d is not needed) -- the profiles of FILE against those of FILE2, or against
// themselves (pairs x < y), at every offset that leaves V [1] columns in common (hs_pssm_compare), after the column
// transform [pearson]; -o holds one line per hit, "<nameX> <nameY> <d> <score %.17g>", in hit order.  Refused:
// --pssm-compare without --pssm or without a threshold, with --pssm-rank, --pssm-refine, --pssm-pvalue, --pssm-top or
// --pssm-per-sequence, files of another -l or alphabet, a V outside 1..-l, any other columns value; and what --pssm refuses.
// --pssm FILE --pssm-families FAM [--pssm-family-blocks C] [--pssm-family-threshold T]: FAM holds one line per profile
// of FILE, "<family> <profile name> <offset>"; the profiles are ordered by (family in order of first appearance, offset,
// file order) and their hits reduced per (family, protein, diagonal) on the device (hs_pssm_family_scan): one line per
// row with at least C [1] profiles in register whose scores add up to T [no such filter], "<family> <protein> <diag>
// <blocks> <sum> <best profile> <best window offset> <best score> <lo> <hi>"; families in FAM order, proteins in
// database order.  Refused: a profile of FILE missing from FAM, one named twice, an unknown name, a malformed line;
// --pssm-top, --pssm-per-sequence, --pssm-compare, --pssm-pvalue-column, --pssm-refine, --pssm-rank or --pssm-pvalue
// beside it; the two companion options without it; a C below 1; a T that is no finite number.
// ... --pssm-families FAM --pssm-family-shift G [--pssm-family-gap-open X] [--pssm-family-gap-extend Y]: instead of the
// rows per diagonal, per (family, protein) the best gapped chain of the family's hits (hs_pssm_family_chain): later
// profiles at later offsets link when their diagonals differ by at most G, at the cost X + Y * d for d >= 1 [0, 0];
// --pssm-family-blocks counts the chain's hits, --pssm-family-threshold bounds its score; "<family> <protein> <blocks>
// <gaps> <score> <first profile> <first offset> <last profile> <last offset> <shift>".  Refused: the two gap options
// without the shift; a G that is no whole number in 0..65535; a penalty that is negative or no finite number; a FAM
// whose offsets decrease inside a family in line order (--pssm-families-out writes an ordered file).
// --pssm-compare self ... --pssm-families-out FAM: that file, written from the comparison's hits (hs_pssm_family_layout);
// the family is named after its first profile; hits that contradict earlier ones are counted on stderr.  Refused
// without --pssm-compare self.
// --pssm-pvalue-column 1: every plain hit line gets " <p_hi>" appended, the upper end of the hit's p-value (hs_pssm_pvalue;
// the grid's floor is the profile's threshold or --pssm-null-floor, whichever is lower); refused with --pssm-top and
// --pssm-per-sequence.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <math.h>

#include <algorithm>
#include <fstream>
#include <iostream>
#include <map>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "hs_host.hpp"

namespace {

struct Opt {
  const char* long_name;
  char short_name;
  const char* descr;
  bool required;
};

const Opt kOpts[] = {
    {"db", 'd', "protein database file (points)", true},
    {"center", 'c', "centers from Pfam database (points)", true},
    {"len", 'l', "kmer length", true},
    {"hash_K", 'K', "number of random lines [4]", false},
    {"hash_L", 'L', "number of hash tables [4]", false},
    {"window", 'W', "bucket width", true},
    {"threshold", 'T', "kmer threshold [REQUIRED unless --radii]", false},
    {"radii", 'r', "file of '<centre name> <radius>' lines: every centre at its own radius (one GPU)", false},
    {"groundtruth", 'g', "groundtruth (sorted brute-force hits); optional", false},
    {"output", 'o', "output file name", true},
    {"seed", 's', "seed of the LSH planes [random_device]", false},
    {"device", 'G', "GPU ordinal (the first one with --gpus) [0]", false},
    {"gpus", 'N', "shard the centres over this many GPUs, hits all-gathered over RCCL [off: one GPU, no communicator]", false},
    {"partition", 'Y', "with --gpus: queries (every GPU the whole index and a block of the centres, the default), tables (every GPU a subset of the L tables over all k-mers and all centres) or buckets (every GPU the whole index, all centres and its share of the buckets); same output", false},
    {"probes", 'M', "multi-probe LSH: look in this many extra buckets per table, 0..63 (points database only) [0]", false},
    {"transport", 'X', "with --gpus: rccl (one rank per GPU, the default) or loopback (host memory between the rank threads, all ranks on --device: the rank protocol on a box with fewer GPUs)", false},
    {"centers-as-points", 'E', "k-mer centres over a FASTA database: send them embedded (8k doubles each) instead of as residue codes [0]", false},
    {"planes", 'p', "read the planes from this file (as written by --planes-out) instead of drawing them", false},
    {"planes-out", 'P', "write the planes (binary doubles a[L][K][d] then b[L][K])", false},
    {"ref-compat-eq-swap", 'Q', "FASTA database: exchange E and Q like the reference's ProteinDB [0]", false},
    {"best-per-position", 'B', "one line per matched database k-mer (FASTA: window), its nearest centre (kmer_search) [0]", false},
    {"per-sequence", 'S', "FASTA database: one line per (centre, protein) with a hit: count, best window, span (one GPU) [0]", false},
    {"query-fasta", 'q', "query proteins in place of -c: one line per (query protein, protein, diagonal) (implies --per-sequence 1)", false},
    {"topk", 't', "per centre only its N best hits, 1..64, in ascending (distance, k-mer index) (one GPU) [off: all hits]", false},
    {"db-append", 'A', "FASTA database: a further FASTA file whose sequences follow -d's, appended to the built index on the GPU; repeatable (one GPU)", false},
    {"pssm", 'm', "FASTA database: scan every window against the position-specific score matrices of this file ('>name threshold', then -l lines of 20 numbers) in place of a search: no -c, -W, -T (one GPU)", false},
    {"pssm-top", 'n', "with --pssm: per profile only its N best windows, 1..64, among those at or above the file's threshold, by descending score then window index [off: every hit]", false},
    {"pssm-per-sequence", 'e', "with --pssm: instead of the hits, one line per (profile, protein) with a hit: count, best window and its score, span; not with --pssm-top [0]", false},
    {"pssm-refine", 'R', "with --pssm and --pssm-out: first rebuild the profiles from their own hits, at most N scans, 1..100; -o then holds what --pssm with the refined file gives [off]", false},
    {"pssm-out", 'O', "with --pssm-refine, --pssm-rank or --pssm-pvalue: write the profiles (refined, with the new thresholds) to this file", false},
    {"pssm-pvalue", 'v', "with --pssm and --pssm-out: replace every threshold by the threshold of this p-value, 0 < P <= 1, under the null model of the database's residue composition; -o then holds what --pssm with that file gives [off]", false},
    {"pssm-null-floor", 'f', "with --pssm-pvalue or --pssm-pvalue-column: the lowest score the null model's grid covers [0; for the column: the profile's threshold if that is lower]", false},
    {"pssm-pvalue-column", 'C', "with --pssm: append the upper end of every hit's p-value to its line; not with --pssm-top or --pssm-per-sequence [0]", false},
    {"pssm-rank", 'k', "with --pssm and --pssm-out: replace every threshold by the score of the profile's N-th best window over the database, 1..windows; -o then holds what --pssm with that file gives [off]", false},
    {"pssm-one-per-protein", 'I', "with --pssm-refine: only the best window of every protein counts [0]", false},
    {"pssm-pseudo", 'u', "with --pssm-refine: pseudo-counts of the log-odds, > 0 [1]", false},
    {"pssm-compare", 'x', "with --pssm and --pssm-compare-threshold: compare the profiles of --pssm with those of this file, or with themselves ('self': pairs x < y), at every offset; one line per hit '<nameX> <nameY> <d> <score>'; no -d", false},
    {"pssm-compare-threshold", 'y', "with --pssm-compare: a pair is a hit when its best offset scores at least this", false},
    {"pssm-compare-overlap", 'z', "with --pssm-compare: the columns two profiles must share at an offset, 1..-l [1]", false},
    {"pssm-compare-columns", 'j', "with --pssm-compare: the column transform applied to both sides first: pearson, cosine or raw [pearson]", false},
    {"pssm-families", 'F', "with --pssm: a file of '<family> <profile name> <offset>' lines, one per profile; instead of the hits, one line per (family, protein, diagonal): blocks in register, the sum of their scores, best block, span (one GPU)", false},
    {"pssm-family-blocks", 'b', "with --pssm-families: report a row only when at least this many of the family's profiles hit on the diagonal, >= 1 [1]", false},
    {"pssm-family-threshold", 'H', "with --pssm-families: report a row only when the scores on the diagonal add up to at least this [off]", false},
    {"pssm-family-shift", 'i', "with --pssm-families: instead of the rows per diagonal, per (family, protein) the best chain of the family's hits whose diagonals differ by at most this between neighbours, 0..65535: '<family> <protein> <blocks> <gaps> <score> <first profile> <first offset> <last profile> <last offset> <shift>' [off]", false},
    {"pssm-family-gap-open", 'a', "with --pssm-family-shift: what a link between two diagonals costs, >= 0 [0]", false},
    {"pssm-family-gap-extend", 'V', "with --pssm-family-shift: ... plus this per diagonal of distance, >= 0 [0]", false},
    {"pssm-families-out", 'J', "with --pssm-compare self: also write the families the hits imply, one '<family> <profile name> <offset>' line per profile, the file --pssm-families reads", false},
    {"pssm-weights", 'w', "with --pssm-refine: weigh the sites with position-based sequence weights; the log-odds count 'sites' or 'columns' (distinct residues per column) as observations [off: every site counts 1]", false},
};

// A points file has a line of numbers after its first name line; a FASTA file has residue letters.
bool LooksLikeFasta(const std::string& path) {
  std::ifstream fin(path.c_str());
  std::string l1, l2;
  if (!std::getline(fin, l1) || l1.empty() || l1[0] != '>') return false;
  while (std::getline(fin, l2))
    if (!l2.empty()) break;
  if (l2.empty()) return false;
  char* end = nullptr;
  (void)strtod(l2.c_str(), &end);
  return end == l2.c_str();  // no number at the start of the second line
}

void Help(const char* prog) {
  fprintf(stderr, "Usage: %s [OPTIONS]\n\nOptions:\n", prog);
  for (const Opt& o : kOpts)
    fprintf(stderr, "  -%c, -%-12s %s%s\n", o.short_name, o.long_name, o.descr,
            o.required ? " [REQUIRED]" : "");
  fprintf(stderr, "\nHelp options:\n  -?, -help   print this help message\n\ncluster kmers to motifs\n");
}

// --pssm: the scan of a FASTA database against position-specific score matrices (hsearch::ScanProfiles).  It is no
// search: what selects, sizes or reduces a search is refused, not ignored.
// what --pssm refuses whatever else is asked
bool PssmRefused(std::map<std::string, std::string>& val, const std::vector<std::string>& db_append) {
  static const struct { const char* name; const char* flag; } kRefused[] = {
      {"center", "-c"}, {"radii", "--radii"}, {"probes", "-M"}, {"topk", "--topk"}, {"per-sequence", "--per-sequence"},
      {"best-per-position", "--best-per-position"}, {"query-fasta", "--query-fasta"}};
  for (const auto& r : kRefused)
    if (val.count(r.name)) {
      fprintf(stderr, "ERROR: --pssm cannot be combined with %s: it scans every window against the profiles, it is "
                      "no search\n", r.flag);
      return true;
    }
  if (val.count("gpus") && atoi(val["gpus"].c_str()) > 1) {
    fprintf(stderr, "ERROR: --pssm runs on one GPU: it cannot be combined with --gpus %s\n", val["gpus"].c_str());
    return true;
  }
  if (!db_append.empty()) {
    fprintf(stderr, "ERROR: --pssm cannot be combined with --db-append\n");
    return true;
  }
  return false;
}

// --pssm FILE --pssm-compare FILE2|self: profiles against profiles (hsearch::CompareProfiles); no database
int CompareMain(std::map<std::string, std::string>& val, const std::vector<std::string>& db_append) {
  if (PssmRefused(val, db_append)) return EXIT_FAILURE;
  for (const char* name : {"pssm-rank", "pssm-refine", "pssm-pvalue", "pssm-top", "pssm-per-sequence", "pssm-out",
                           "pssm-pvalue-column", "pssm-null-floor"})
    if (val.count(name)) {
      fprintf(stderr, "ERROR: --pssm-compare compares profiles with profiles: it cannot be combined with --%s\n", name);
      return EXIT_FAILURE;
    }
  if (!val.count("pssm-compare-threshold")) {
    fprintf(stderr, "ERROR: --pssm-compare needs --pssm-compare-threshold: the score a pair's best offset must reach\n");
    return EXIT_FAILURE;
  }
  char* end = nullptr;
  const std::string& ttext = val["pssm-compare-threshold"];
  const double threshold = strtod(ttext.c_str(), &end);
  if (ttext.empty() || end == ttext.c_str() || *end || !(fabs(threshold) <= 1.7976931348623157e308)) {
    fprintf(stderr, "ERROR: --pssm-compare-threshold takes a finite score\n");
    return EXIT_FAILURE;
  }
  const uint32_t kmer_length = (uint32_t)strtoul(val["len"].c_str(), nullptr, 10);
  uint32_t overlap = 1;
  if (val.count("pssm-compare-overlap")) {
    const std::string& text = val["pssm-compare-overlap"];
    const long v = strtol(text.c_str(), &end, 10);
    if (text.empty() || end == text.c_str() || *end || v < 1 || v > (long)kmer_length) {
      fprintf(stderr, "ERROR: --pssm-compare-overlap takes a number of columns, 1..%u\n", kmer_length);
      return EXIT_FAILURE;
    }
    overlap = (uint32_t)v;
  }
  int columns = 0;
  if (val.count("pssm-compare-columns")) {
    const std::string& text = val["pssm-compare-columns"];
    if (text != "pearson" && text != "cosine" && text != "raw") {
      fprintf(stderr, "ERROR: --pssm-compare-columns takes 'pearson', 'cosine' or 'raw'\n");
      return EXIT_FAILURE;
    }
    columns = text == "pearson" ? 0 : text == "cosine" ? 1 : -1;
  }
  const int device = val.count("device") ? atoi(val["device"].c_str()) : 0;
  try {
    std::vector<std::string> names_x, names_y;
    std::vector<double> X, Y, t_file;
    std::string err;
    if (!hsearch::ReadPssmFile(val["pssm"], kmer_length, &names_x, &X, &t_file, &err)) {
      fprintf(stderr, "ERROR: %s\n", err.c_str());
      return EXIT_FAILURE;
    }
    const bool self = val["pssm-compare"] == "self";
    if (!self && !hsearch::ReadPssmFile(val["pssm-compare"], kmer_length, &names_y, &Y, &t_file, &err)) {
      fprintf(stderr, "ERROR: %s\n", err.c_str());
      return EXIT_FAILURE;
    }
    std::cout << "number of profiles " << names_x.size();
    if (!self) std::cout << " against " << names_y.size();
    std::cout << std::endl;
    const std::vector<double> t(names_x.size(), threshold);
    uint64_t n_hits = 0, n_families = 0, n_conflicts = 0;
    const bool families = val.count("pssm-families-out") != 0;
    if (families && !self) {
      fprintf(stderr, "ERROR: --pssm-families-out lays out the profiles of one file: it needs --pssm-compare self\n");
      return EXIT_FAILURE;
    }
    const int st = hsearch::CompareProfiles(kmer_length, names_x, X, t, self ? nullptr : &names_y, self ? nullptr : &Y,
                                            overlap, columns, val["output"], device, &err, &n_hits,
                                            families ? &val["pssm-families-out"] : nullptr, &n_families, &n_conflicts);
    if (st != 0) {
      fprintf(stderr, "ERROR: %s (status %d)\n", err.c_str(), st);
      return EXIT_FAILURE;
    }
    std::cout << "number of hits " << n_hits << std::endl;
    if (families) {
      std::cout << "number of families " << n_families << std::endl;
      if (n_conflicts) fprintf(stderr, "NOTE: %llu hits contradict the offsets fixed by earlier hits\n", (unsigned long long)n_conflicts);
    }
  } catch (const std::bad_alloc&) {
    fprintf(stderr, "ERROR: could not allocate memory\n");
    return EXIT_FAILURE;
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}

// --pssm FILE --pssm-families FAM: the profiles' hits per (family, protein, diagonal) (hsearch::FamilyScan)
int FamilyMain(std::map<std::string, std::string>& val, const std::vector<std::string>& db_append) {
  if (PssmRefused(val, db_append)) return EXIT_FAILURE;
  for (const char* name : {"pssm-top", "pssm-per-sequence", "pssm-compare", "pssm-pvalue-column", "pssm-refine",
                           "pssm-rank", "pssm-pvalue", "pssm-out", "pssm-null-floor", "pssm-families-out"})
    if (val.count(name)) {
      fprintf(stderr, "ERROR: --pssm-families reduces the hits per family: it cannot be combined with --%s\n", name);
      return EXIT_FAILURE;
    }
  char* end = nullptr;
  uint32_t blocks = 1;
  if (val.count("pssm-family-blocks")) {
    const std::string& text = val["pssm-family-blocks"];
    const long long v = strtoll(text.c_str(), &end, 10);
    if (text.empty() || end == text.c_str() || *end || v < 1 || v > 0xffffffffll) {
      fprintf(stderr, "ERROR: --pssm-family-blocks takes a number of profiles, 1 or more\n");
      return EXIT_FAILURE;
    }
    blocks = (uint32_t)v;
  }
  double threshold = 0.0;
  const bool with_threshold = val.count("pssm-family-threshold") != 0;
  if (with_threshold) {
    const std::string& text = val["pssm-family-threshold"];
    threshold = strtod(text.c_str(), &end);
    if (text.empty() || end == text.c_str() || *end || !(fabs(threshold) <= 1.7976931348623157e308)) {
      fprintf(stderr, "ERROR: --pssm-family-threshold takes a finite score\n");
      return EXIT_FAILURE;
    }
  }
  const bool with_chain = val.count("pssm-family-shift") != 0;
  uint32_t max_shift = 0;
  double gap_open = 0.0, gap_ext = 0.0;
  if (with_chain) {
    const std::string& text = val["pssm-family-shift"];
    const long long v = strtoll(text.c_str(), &end, 10);
    if (text.empty() || end == text.c_str() || *end || text[0] == '+' || v < 0 || v > 65535) {
      fprintf(stderr, "ERROR: --pssm-family-shift takes a whole number of diagonals, 0 .. 65535\n");
      return EXIT_FAILURE;
    }
    max_shift = (uint32_t)v;
    const std::pair<const char*, double*> gaps[2] = {{"pssm-family-gap-open", &gap_open},
                                                     {"pssm-family-gap-extend", &gap_ext}};
    for (const auto& g : gaps) {
      if (!val.count(g.first)) continue;
      const std::string& gt = val[g.first];
      *g.second = strtod(gt.c_str(), &end);
      if (gt.empty() || end == gt.c_str() || *end || !(*g.second >= 0.0) || !(*g.second <= 1.7976931348623157e308)) {
        fprintf(stderr, "ERROR: --%s takes a finite penalty, 0 or more\n", g.first);
        return EXIT_FAILURE;
      }
    }
  }
  const uint32_t kmer_length = (uint32_t)strtoul(val["len"].c_str(), nullptr, 10);
  const int device = val.count("device") ? atoi(val["device"].c_str()) : 0;
  try {
    if (!LooksLikeFasta(val["db"])) {
      fprintf(stderr, "ERROR: --pssm needs a FASTA database: a points database holds no residues\n");
      return EXIT_FAILURE;
    }
    std::vector<std::string> names;
    std::vector<double> S, t;
    std::string err;
    if (!hsearch::ReadPssmFile(val["pssm"], kmer_length, &names, &S, &t, &err)) {
      fprintf(stderr, "ERROR: %s\n", err.c_str());
      return EXIT_FAILURE;
    }
    std::map<std::string, uint32_t> last_offset;  // per family, in line order
    // FAM: every profile of FILE once, with its family and offset
    const size_t nm = names.size();
    std::map<std::string, size_t> index_of;
    for (size_t m = 0; m < nm; ++m) index_of[names[m]] = m;
    std::vector<std::string> family(nm), fam_order;
    std::vector<uint32_t> offset(nm, 0);
    std::vector<char> seen(nm, 0);
    std::ifstream fam(val["pssm-families"].c_str());
    if (!fam) {
      fprintf(stderr, "ERROR: cannot open %s\n", val["pssm-families"].c_str());
      return EXIT_FAILURE;
    }
    std::string line;
    for (size_t ln = 1; std::getline(fam, line); ++ln) {
      std::istringstream in(line);
      std::string f, name, off, rest;
      if (!(in >> f)) continue;  // an empty line
      const bool three = bool(in >> name >> off) && !(in >> rest);
      const unsigned long long v = three ? strtoull(off.c_str(), &end, 10) : 0;
      if (!three || off[0] == '-' || end == off.c_str() || *end || v > 0x7fffffffull) {
        fprintf(stderr, "ERROR: %s line %zu: expected '<family> <profile name> <offset>', the offset 0 .. 2^31 - 1\n",
                val["pssm-families"].c_str(), ln);
        return EXIT_FAILURE;
      }
      const auto it = index_of.find(name);
      if (it == index_of.end()) {
        fprintf(stderr, "ERROR: %s line %zu: %s names no profile of %s\n", val["pssm-families"].c_str(), ln,
                name.c_str(), val["pssm"].c_str());
        return EXIT_FAILURE;
      }
      if (seen[it->second]) {
        fprintf(stderr, "ERROR: %s line %zu: profile %s is named twice\n", val["pssm-families"].c_str(), ln, name.c_str());
        return EXIT_FAILURE;
      }
      if (with_chain && last_offset.count(f) && (uint32_t)v < last_offset[f]) {
        fprintf(stderr,
                "ERROR: %s line %zu: the offsets of family %s decrease; --pssm-family-shift takes a family's profiles "
                "in block order (--pssm-compare self --pssm-families-out writes an ordered file)\n",
                val["pssm-families"].c_str(), ln, f.c_str());
        return EXIT_FAILURE;
      }
      last_offset[f] = (uint32_t)v;
      seen[it->second] = 1;
      family[it->second] = f;
      offset[it->second] = (uint32_t)v;
      if (std::find(fam_order.begin(), fam_order.end(), f) == fam_order.end()) fam_order.push_back(f);
    }
    for (size_t m = 0; m < nm; ++m)
      if (!seen[m]) {
        fprintf(stderr, "ERROR: profile %s of %s is missing from %s\n", names[m].c_str(), val["pssm"].c_str(),
                val["pssm-families"].c_str());
        return EXIT_FAILURE;
      }
    // by (family in order of first appearance, offset, file order)
    std::map<std::string, size_t> fam_rank;
    for (size_t i = 0; i < fam_order.size(); ++i) fam_rank[fam_order[i]] = i;
    std::vector<size_t> order(nm);
    for (size_t m = 0; m < nm; ++m) order[m] = m;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
      if (fam_rank[family[a]] != fam_rank[family[b]]) return fam_rank[family[a]] < fam_rank[family[b]];
      if (offset[a] != offset[b]) return offset[a] < offset[b];
      return a < b;
    });
    const size_t ka = (size_t)kmer_length * 20;
    std::vector<std::string> names2(nm), family2(nm);
    std::vector<double> S2(S.size()), t2(nm);
    std::vector<uint32_t> offset2(nm);
    for (size_t i = 0; i < nm; ++i) {
      const size_t m = order[i];
      names2[i] = names[m];
      family2[i] = family[m];
      offset2[i] = offset[m];
      t2[i] = t[m];
      std::copy(S.begin() + m * ka, S.begin() + (m + 1) * ka, S2.begin() + i * ka);
    }
    hsearch::ProteinDB prodb;
    std::cout << "Read protein sequences from " << val["db"] << std::endl;
    const bool swap = val.count("ref-compat-eq-swap") && atoi(val["ref-compat-eq-swap"].c_str()) != 0;
    if (!hsearch::ReadProteinFasta(val["db"], swap, &prodb)) {
      fprintf(stderr, "cannot open %s\n", val["db"].c_str());
      return EXIT_FAILURE;
    }
    std::cout << "number of proteins " << prodb.start.size() - 1 << std::endl;
    std::cout << "total length " << prodb.residues.size() << std::endl;
    std::cout << "number of profiles " << nm << " in " << fam_order.size() << " families" << std::endl;
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    uint64_t n_windows = 0, n_hits = 0, n_rows = 0;
    const int st =
        with_chain ? hsearch::FamilyChain(prodb, kmer_length, names2, S2, t2, family2, offset2, max_shift, gap_open,
                                          gap_ext, blocks, with_threshold ? &threshold : nullptr, val["output"], device,
                                          &err, &n_windows, &n_hits, &n_rows)
                   : hsearch::FamilyScan(prodb, kmer_length, names2, S2, t2, family2, offset2, blocks,
                                         with_threshold ? &threshold : nullptr, val["output"], device, &err, &n_windows,
                                         &n_hits, &n_rows);
    if (st != 0) {
      fprintf(stderr, "ERROR: %s (status %d)\n", err.c_str(), st);
      return EXIT_FAILURE;
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    std::cout << "number of kmers " << n_windows << std::endl;
    std::cout << "number of hits " << n_hits << std::endl;
    std::cout << "number of rows " << n_rows << std::endl;
    printf("SCAN: %lf seconds\n", (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec));
  } catch (const std::bad_alloc&) {
    fprintf(stderr, "ERROR: could not allocate memory\n");
    return EXIT_FAILURE;
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}

int PssmMain(std::map<std::string, std::string>& val, const std::vector<std::string>& db_append) {
  if (PssmRefused(val, db_append)) return EXIT_FAILURE;
  uint32_t top_n = 0;  // 0: every hit
  if (val.count("pssm-top")) {
    char* end = nullptr;
    const long v = strtol(val["pssm-top"].c_str(), &end, 10);
    if (end == val["pssm-top"].c_str() || *end || v < 1 || v > 64) {
      fprintf(stderr, "ERROR: --pssm-top takes a number of lines per profile, 1..64\n");
      return EXIT_FAILURE;
    }
    top_n = (uint32_t)v;
  }
  const bool per_sequence = val.count("pssm-per-sequence") && atoi(val["pssm-per-sequence"].c_str()) != 0;
  if (per_sequence && top_n) {
    fprintf(stderr, "ERROR: --pssm-per-sequence reduces every hit of a profile: it cannot be combined with --pssm-top\n");
    return EXIT_FAILURE;
  }
  uint32_t refine = 0;  // 0: the profiles as the file gives them
  double pseudo = 1.0;
  if (val.count("pssm-refine")) {
    char* end = nullptr;
    const long v = strtol(val["pssm-refine"].c_str(), &end, 10);
    if (end == val["pssm-refine"].c_str() || *end || v < 1 || v > 100) {
      fprintf(stderr, "ERROR: --pssm-refine takes a number of scans, 1..100\n");
      return EXIT_FAILURE;
    }
    refine = (uint32_t)v;
    if (!val.count("pssm-out")) {
      fprintf(stderr, "ERROR: --pssm-refine needs --pssm-out: the file the refined profiles are written to\n");
      return EXIT_FAILURE;
    }
    if (val.count("pssm-pseudo")) {
      pseudo = strtod(val["pssm-pseudo"].c_str(), &end);
      if (end == val["pssm-pseudo"].c_str() || *end || !(pseudo > 0.0) || !(pseudo <= 1.7976931348623157e308)) {
        fprintf(stderr, "ERROR: --pssm-pseudo takes a finite number above 0\n");
        return EXIT_FAILURE;
      }
    }
  }
  int weights = -1;  // -1: every site counts 1; 0: weighted, n_eff = the sites; 1: n_eff = distinct residues per column
  if (val.count("pssm-weights")) {
    weights = val["pssm-weights"] == "sites" ? 0 : val["pssm-weights"] == "columns" ? 1 : -1;
    if (weights < 0) {
      fprintf(stderr, "ERROR: --pssm-weights takes 'sites' or 'columns'\n");
      return EXIT_FAILURE;
    }
  }  // (main has refused --pssm-weights without --pssm-refine)
  uint64_t rank_n = 0;  // 0: the thresholds as the file gives them
  if (val.count("pssm-rank")) {
    const std::string& text = val["pssm-rank"];
    char* end = nullptr;
    const unsigned long long v = strtoull(text.c_str(), &end, 10);
    if (text.empty() || text.find_first_not_of("0123456789") != std::string::npos || *end || v < 1 ||
        v > 0xffffffffull) {
      fprintf(stderr, "ERROR: --pssm-rank takes a whole number of windows, 1 .. the windows of the database\n");
      return EXIT_FAILURE;
    }
    rank_n = v;
    if (!val.count("pssm-out")) {
      fprintf(stderr, "ERROR: --pssm-rank needs --pssm-out: the file the profiles and their new thresholds are written to\n");
      return EXIT_FAILURE;
    }
  }
  double pvalue = 0.0, null_floor = 0.0;  // pvalue 0: the thresholds as the file gives them
  const bool with_floor = val.count("pssm-null-floor") != 0;
  const bool pvalue_column = val.count("pssm-pvalue-column") && atoi(val["pssm-pvalue-column"].c_str()) != 0;
  if (val.count("pssm-pvalue")) {
    const std::string& text = val["pssm-pvalue"];
    char* end = nullptr;
    pvalue = strtod(text.c_str(), &end);
    if (text.empty() || end == text.c_str() || *end || !(pvalue > 0.0) || !(pvalue <= 1.0)) {
      fprintf(stderr, "ERROR: --pssm-pvalue takes a probability, 0 < P <= 1\n");
      return EXIT_FAILURE;
    }
    if (!val.count("pssm-out")) {
      fprintf(stderr, "ERROR: --pssm-pvalue needs --pssm-out: the file the profiles and their new thresholds are written to\n");
      return EXIT_FAILURE;
    }
    if (rank_n || refine) {
      fprintf(stderr, "ERROR: --pssm-pvalue sets the thresholds from a null model: it cannot be combined with %s\n",
              rank_n ? "--pssm-rank" : "--pssm-refine");
      return EXIT_FAILURE;
    }
  }
  if (pvalue_column && (top_n || per_sequence)) {
    fprintf(stderr, "ERROR: --pssm-pvalue-column belongs to the plain hit lines: it cannot be combined with %s\n",
            top_n ? "--pssm-top" : "--pssm-per-sequence");
    return EXIT_FAILURE;
  }
  if (with_floor) {
    const std::string& text = val["pssm-null-floor"];
    char* end = nullptr;
    null_floor = strtod(text.c_str(), &end);
    if (text.empty() || end == text.c_str() || *end || !(fabs(null_floor) <= 1.7976931348623157e308)) {
      fprintf(stderr, "ERROR: --pssm-null-floor takes a finite score\n");
      return EXIT_FAILURE;
    }
    if (!(pvalue > 0.0) && !pvalue_column) {
      fprintf(stderr, "ERROR: --pssm-null-floor belongs to --pssm-pvalue or --pssm-pvalue-column: it cannot be given without them\n");
      return EXIT_FAILURE;
    }
  }
  const bool one_per_protein = val.count("pssm-one-per-protein") && atoi(val["pssm-one-per-protein"].c_str()) != 0;
  const uint32_t kmer_length = (uint32_t)strtoul(val["len"].c_str(), nullptr, 10);
  const int device = val.count("device") ? atoi(val["device"].c_str()) : 0;
  try {
    if (!LooksLikeFasta(val["db"])) {
      fprintf(stderr, "ERROR: --pssm needs a FASTA database: a points database holds no residues\n");
      return EXIT_FAILURE;
    }
    hsearch::ProteinDB prodb;
    std::cout << "Read protein sequences from " << val["db"] << std::endl;
    const bool swap = val.count("ref-compat-eq-swap") && atoi(val["ref-compat-eq-swap"].c_str()) != 0;
    if (!hsearch::ReadProteinFasta(val["db"], swap, &prodb)) {
      fprintf(stderr, "cannot open %s\n", val["db"].c_str());
      return EXIT_FAILURE;
    }
    std::cout << "number of proteins " << prodb.start.size() - 1 << std::endl;
    std::cout << "total length " << prodb.residues.size() << std::endl;
    std::vector<std::string> names;
    std::vector<double> S, t;
    std::string err;
    if (!hsearch::ReadPssmFile(val["pssm"], kmer_length, &names, &S, &t, &err)) {
      fprintf(stderr, "ERROR: %s\n", err.c_str());
      return EXIT_FAILURE;
    }
    std::cout << "number of profiles " << names.size() << std::endl;
    // (a rank above the database's windows is refused by the library, with nothing written)
    const std::vector<uint64_t> ranks(names.size(), rank_n);
    if (rank_n && !refine) {
      std::vector<double> t_rank;
      const int rst = hsearch::RankThresholds(prodb, kmer_length, S, ranks, device, &t_rank, nullptr, nullptr, &err);
      if (rst != 0) {
        fprintf(stderr, "ERROR: %s (status %d)\n", err.c_str(), rst);
        return EXIT_FAILURE;
      }
      t.swap(t_rank);
      if (!hsearch::WritePssmFile(val["pssm-out"], kmer_length, names, S, t, &err)) {
        fprintf(stderr, "ERROR: %s\n", err.c_str());
        return EXIT_FAILURE;
      }
      std::cout << "thresholds set to the score of rank " << rank_n << std::endl;
    }
    if (pvalue > 0.0) {
      const std::vector<double> ps(names.size(), pvalue), floors(names.size(), null_floor);
      std::vector<double> t_p;
      std::vector<uint32_t> flag;
      const int pst = hsearch::PvalueThresholds(prodb, kmer_length, S, ps, floors, device, &t_p, nullptr, nullptr, &flag, &err);
      if (pst != 0) {
        fprintf(stderr, "ERROR: %s (status %d)\n", err.c_str(), pst);
        return EXIT_FAILURE;
      }
      t.swap(t_p);
      for (size_t m = 0; m < names.size(); ++m) {
        if (flag[m] == 1)
          fprintf(stderr, "NOTE: profile %s: the threshold is clipped at the floor %.17g; a lower --pssm-null-floor may admit more\n",
                  names[m].c_str(), null_floor);
        if (flag[m] == 2)
          fprintf(stderr, "NOTE: profile %s: no score has a p-value of at most %.17g; it keeps +DBL_MAX and finds nothing\n",
                  names[m].c_str(), pvalue);
      }
      if (!hsearch::WritePssmFile(val["pssm-out"], kmer_length, names, S, t, &err)) {
        fprintf(stderr, "ERROR: %s\n", err.c_str());
        return EXIT_FAILURE;
      }
      std::cout << "thresholds set to the p-value " << pvalue << std::endl;
    }
    if (refine) {
      std::vector<double> refined, t_last;
      uint32_t iters = 0;
      bool converged = false;
      const int rst = weights >= 0 ? hsearch::RefineProfilesWeighted(prodb, kmer_length, S, rank_n ? nullptr : &t,
                                                                     rank_n ? &ranks : nullptr, weights == 1, refine,
                                                                     one_per_protein, pseudo, device, &refined, &t_last,
                                                                     &iters, &converged, &err)
                      : rank_n ? hsearch::RefineProfiles(prodb, kmer_length, S, ranks, refine, one_per_protein, pseudo,
                                                         device, &refined, &t_last, &iters, &converged, &err)
                               : hsearch::RefineProfiles(prodb, kmer_length, S, t, refine, one_per_protein, pseudo, device,
                                                         &refined, &iters, &converged, &err);
      if (rank_n && rst == 0) t.swap(t_last);
      if (rst != 0) {
        fprintf(stderr, "ERROR: %s (status %d)\n", err.c_str(), rst);
        return EXIT_FAILURE;
      }
      S.swap(refined);
      if (!hsearch::WritePssmFile(val["pssm-out"], kmer_length, names, S, t, &err)) {
        fprintf(stderr, "ERROR: %s\n", err.c_str());
        return EXIT_FAILURE;
      }
      std::cout << "refined in " << iters << " scans" << (converged ? " (converged)" : "") << std::endl;
    }
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    uint64_t n_windows = 0, n_hits = 0, n_rows = 0;
    std::vector<double> column_floor(t);  // the column's grid: from the threshold, or from the floor if that is lower
    for (double& f : column_floor)
      if (with_floor && null_floor < f) f = null_floor;
    const int st = per_sequence ? hsearch::ScanProfilesPerSequence(prodb, kmer_length, names, S, t, val["output"], device,
                                                                   &err, &n_windows, &n_hits, &n_rows)
                   : pvalue_column ? hsearch::HitPvalues(prodb, kmer_length, names, S, t, column_floor, val["output"], device,
                                                         &err, &n_windows, &n_hits)
                   : top_n ? hsearch::ScanProfilesTopN(prodb, kmer_length, names, S, t, top_n, val["output"], device, &err,
                                                       &n_windows, &n_hits)
                           : hsearch::ScanProfiles(prodb, kmer_length, names, S, t, val["output"], device, &err,
                                                   &n_windows, &n_hits);
    if (st != 0) {
      fprintf(stderr, "ERROR: %s (status %d)\n", err.c_str(), st);
      return EXIT_FAILURE;
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    std::cout << "number of kmers " << n_windows << std::endl;
    std::cout << "number of hits " << n_hits << std::endl;
    if (per_sequence) std::cout << "number of rows " << n_rows << std::endl;
    printf("SCAN: %lf seconds\n", (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec));
  } catch (const std::bad_alloc&) {
    fprintf(stderr, "ERROR: could not allocate memory\n");
    return EXIT_FAILURE;
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}

}  // namespace

int main(int argc, const char* argv[]) {
  bool help = false;
  std::map<std::string, std::string> val;
  std::vector<std::string> db_append;  // --db-append, in order
  for (int i = 1; i < argc; ++i) {
    std::string arg = argv[i];
    if (arg == "-help" || arg == "--help" || arg == "-?" || arg == "-about") {
      help = true;
      continue;
    }
    if (arg.size() < 2 || arg[0] != '-') continue;  // leftover argument, ignored like the reference
    std::string name = arg.substr(arg[1] == '-' ? 2 : 1);
    const Opt* hit = nullptr;
    for (const Opt& o : kOpts)
      if (name == o.long_name || (name.size() == 1 && name[0] == o.short_name)) hit = &o;
    if (!hit) {
      fprintf(stderr, "unknown option %s\n", arg.c_str());
      return EXIT_FAILURE;
    }
    if (i + 1 >= argc) {
      fprintf(stderr, "option %s needs a value\n", arg.c_str());
      return EXIT_FAILURE;
    }
    val[hit->long_name] = argv[++i];
    if (std::string(hit->long_name) == "db-append") db_append.push_back(argv[i]);
  }
  if (argc > 1 && !help) {
    fprintf(stdout, "[WELCOME TO HSEARCH v1.0 -- MI355X]\n[%s", argv[0]);
    for (int i = 1; i < argc; ++i) fprintf(stdout, " %s", argv[i]);
    fprintf(stdout, "]\n");
  }
  if (argc == 1 || help) {
    Help(argv[0]);
    return EXIT_SUCCESS;
  }
  const bool query_fasta = val.count("query-fasta") != 0;
  const bool with_pssm = val.count("pssm") != 0;
  if (val.count("pssm-top") && !with_pssm) {
    fprintf(stderr, "ERROR: --pssm-top selects among the hits of --pssm: it cannot be given without it\n");
    return EXIT_FAILURE;
  }
  if (val.count("pssm-per-sequence") && !with_pssm) {
    fprintf(stderr, "ERROR: --pssm-per-sequence reduces the hits of --pssm: it cannot be given without it\n");
    return EXIT_FAILURE;
  }
  for (const char* name : {"pssm-pvalue", "pssm-null-floor", "pssm-pvalue-column"})
    if (val.count(name) && !with_pssm) {
      fprintf(stderr, "ERROR: --%s belongs to --pssm FILE: it cannot be given without it\n", name);
      return EXIT_FAILURE;
    }
  const bool with_compare = val.count("pssm-compare") != 0;
  if (with_compare && !with_pssm) {
    fprintf(stderr, "ERROR: --pssm-compare compares the profiles of --pssm FILE: it cannot be given without it\n");
    return EXIT_FAILURE;
  }
  for (const char* name : {"pssm-compare-threshold", "pssm-compare-overlap", "pssm-compare-columns"})
    if (val.count(name) && !with_compare) {
      fprintf(stderr, "ERROR: --%s belongs to --pssm-compare: it cannot be given without it\n", name);
      return EXIT_FAILURE;
    }
  const bool with_families = val.count("pssm-families") != 0;
  if (with_families && !with_pssm) {
    fprintf(stderr, "ERROR: --pssm-families groups the profiles of --pssm FILE: it cannot be given without it\n");
    return EXIT_FAILURE;
  }
  for (const char* name : {"pssm-family-blocks", "pssm-family-threshold"})
    if (val.count(name) && !with_families) {
      fprintf(stderr, "ERROR: --%s belongs to --pssm-families: it cannot be given without it\n", name);
      return EXIT_FAILURE;
    }
  for (const char* name : {"pssm-family-gap-open", "pssm-family-gap-extend"})
    if (val.count(name) && !val.count("pssm-family-shift")) {
      fprintf(stderr, "ERROR: --%s belongs to --pssm-family-shift: it cannot be given without it\n", name);
      return EXIT_FAILURE;
    }
  if (val.count("pssm-family-shift") && !with_families) {
    fprintf(stderr, "ERROR: --pssm-family-shift belongs to --pssm-families: it cannot be given without it\n");
    return EXIT_FAILURE;
  }
  if (val.count("pssm-families-out") && !with_compare) {
    fprintf(stderr, "ERROR: --pssm-families-out belongs to --pssm-compare self: it cannot be given without it\n");
    return EXIT_FAILURE;
  }
  if (val.count("pssm-rank") && !with_pssm) {
    fprintf(stderr, "ERROR: --pssm-rank sets the thresholds of --pssm FILE: it cannot be given without it\n");
    return EXIT_FAILURE;
  }
  for (const char* name : {"pssm-refine", "pssm-out", "pssm-one-per-protein", "pssm-pseudo", "pssm-weights"})
    if (val.count(name) && !(with_pssm && (val.count("pssm-refine") ||
                                           (std::string(name) == "pssm-out" &&
                                            (val.count("pssm-rank") || val.count("pssm-pvalue")))))) {
      fprintf(stderr, "ERROR: --%s belongs to --pssm FILE --pssm-refine N --pssm-out FILE2: it cannot be given without them\n",
              name);
      return EXIT_FAILURE;
    }
  const bool per_sequence = query_fasta || (val.count("per-sequence") && atoi(val["per-sequence"].c_str()) != 0);
  for (const Opt& o : kOpts)
    if (o.required && !val.count(o.long_name) && !(query_fasta && std::string(o.long_name) == "center") &&
        !(with_pssm && (std::string(o.long_name) == "center" || std::string(o.long_name) == "window")) &&
        !(with_compare && std::string(o.long_name) == "db")) {
      fprintf(stderr, "missing required option -%c\n", o.short_name);
      Help(argv[0]);
      return EXIT_SUCCESS;  // as the reference: option_missing() -> message, EXIT_SUCCESS
    }
  if (with_families) return FamilyMain(val, db_append);
  if (with_compare) return CompareMain(val, db_append);
  if (with_pssm) return PssmMain(val, db_append);
  const bool with_radii = val.count("radii") != 0;
  if (!with_radii && !val.count("threshold")) {
    fprintf(stderr, "missing required option -T\n");
    Help(argv[0]);
    return EXIT_SUCCESS;
  }
  if (with_radii && val.count("gpus") && atoi(val["gpus"].c_str()) > 1) {
    fprintf(stderr, "ERROR: --radii runs on one GPU: it cannot be combined with --gpus %s\n", val["gpus"].c_str());
    return EXIT_FAILURE;
  }
  if (with_radii && val.count("threshold")) fprintf(stderr, "--radii given: -T is ignored\n");
  if (!db_append.empty() && val.count("gpus") && atoi(val["gpus"].c_str()) > 1) {
    fprintf(stderr, "ERROR: --db-append runs on one GPU: it cannot be combined with --gpus %s\n", val["gpus"].c_str());
    return EXIT_FAILURE;
  }
  uint32_t topk = 0;  // 0: all hits
  if (val.count("topk")) {
    char* end = nullptr;
    const unsigned long long t = strtoull(val["topk"].c_str(), &end, 10);
    if (end == val["topk"].c_str() || *end || t < 1 || t > 64 || val["topk"][0] == '-') {
      fprintf(stderr, "ERROR: --topk must be a whole number 1..64, not '%s'\n", val["topk"].c_str());
      return EXIT_FAILURE;
    }
    topk = (uint32_t)t;
    if (val.count("gpus") && atoi(val["gpus"].c_str()) > 1) {
      fprintf(stderr, "ERROR: --topk runs on one GPU: it cannot be combined with --gpus %s\n", val["gpus"].c_str());
      return EXIT_FAILURE;
    }
    if (val.count("best-per-position") && atoi(val["best-per-position"].c_str()) != 0) {
      fprintf(stderr, "ERROR: --topk cannot be combined with --best-per-position %s: an annotation has one line per "
                      "k-mer\n", val["best-per-position"].c_str());
      return EXIT_FAILURE;
    }
  }
  if (per_sequence) {
    const char* flag = query_fasta ? "--query-fasta" : "--per-sequence";
    if (query_fasta && val.count("center")) {
      fprintf(stderr, "ERROR: --query-fasta takes the place of -c: give one of them\n");
      return EXIT_FAILURE;
    }
    if (val.count("gpus") && atoi(val["gpus"].c_str()) > 1) {
      fprintf(stderr, "ERROR: %s runs on one GPU: it cannot be combined with --gpus %s\n", flag, val["gpus"].c_str());
      return EXIT_FAILURE;
    }
    if (topk) {
      fprintf(stderr, "ERROR: %s cannot be combined with --topk %u: its lines are per protein, not per hit\n", flag, topk);
      return EXIT_FAILURE;
    }
    if (val.count("best-per-position") && atoi(val["best-per-position"].c_str()) != 0) {
      fprintf(stderr, "ERROR: %s cannot be combined with --best-per-position %s: an annotation has one line per k-mer\n",
              flag, val["best-per-position"].c_str());
      return EXIT_FAILURE;
    }
  }
  const uint32_t kmer_length = (uint32_t)strtoul(val["len"].c_str(), nullptr, 10);
  const uint32_t hash_K = val.count("hash_K") ? (uint32_t)strtoul(val["hash_K"].c_str(), nullptr, 10) : 4;
  const uint32_t hash_L = val.count("hash_L") ? (uint32_t)strtoul(val["hash_L"].c_str(), nullptr, 10) : 4;
  const double hash_W = strtod(val["window"].c_str(), nullptr);
  double hash_R = with_radii ? 0.0 : strtod(val["threshold"].c_str(), nullptr);
  const int device = val.count("device") ? atoi(val["device"].c_str()) : 0;
  const uint32_t dim = 8 * kmer_length;
  uint32_t seed;
  if (val.count("seed")) {
    seed = (uint32_t)strtoul(val["seed"].c_str(), nullptr, 10);
  } else {
    std::random_device rd;
    seed = rd();
  }
  try {
    std::vector<std::string> kmer_names, center_names;
    std::vector<hsearch::Point> kmers, centers;
    std::vector<uint8_t> center_codes;  // -c <k-mers.fa>: the centres as rows of the coordinate table
    const bool fasta_db = LooksLikeFasta(val["db"]);
    if (!db_append.empty() && !fasta_db) {
      fprintf(stderr, "ERROR: --db-append needs a FASTA database: a points database cannot be appended to\n");
      return EXIT_FAILURE;
    }
    hsearch::ProteinDB prodb;
    if (fasta_db) {
      std::cout << "Read protein sequences from " << val["db"] << std::endl;
      const bool swap = val.count("ref-compat-eq-swap") && atoi(val["ref-compat-eq-swap"].c_str()) != 0;
      if (!hsearch::ReadProteinFasta(val["db"], swap, &prodb)) {
        fprintf(stderr, "cannot open %s\n", val["db"].c_str());
        return EXIT_FAILURE;
      }
      std::cout << "number of proteins " << prodb.start.size() - 1 << std::endl;
      std::cout << "total length " << prodb.residues.size() << std::endl;
    } else {
      std::cout << "Read Kmers..." << std::endl;
      if (!hsearch::ReadPointsFile(val["db"], dim, &kmer_names, &kmers)) {
        fprintf(stderr, "cannot open %s\n", val["db"].c_str());
        return EXIT_FAILURE;
      }
    }
    std::vector<hsearch::ProteinDB> more(db_append.size());
    for (size_t i = 0; i < db_append.size(); ++i) {
      std::cout << "Read appended protein sequences from " << db_append[i] << std::endl;
      if (!LooksLikeFasta(db_append[i]) || !hsearch::ReadProteinFasta(db_append[i], prodb.eq_swapped, &more[i])) {
        fprintf(stderr, "ERROR: --db-append %s: cannot open it, or it is no FASTA file\n", db_append[i].c_str());
        return EXIT_FAILURE;
      }
    }
    if (per_sequence && !fasta_db) {
      fprintf(stderr, "ERROR: --per-sequence / --query-fasta need a FASTA database: a points file names no proteins\n");
      return EXIT_FAILURE;
    }
    hsearch::ProteinDB qrydb;
    if (query_fasta) {
      std::cout << "Read query proteins from " << val["query-fasta"] << std::endl;
      if (!hsearch::ReadProteinFasta(val["query-fasta"], prodb.eq_swapped, &qrydb)) {
        fprintf(stderr, "cannot open %s\n", val["query-fasta"].c_str());
        return EXIT_FAILURE;
      }
      center_names = qrydb.name;  // (what --radii names)
      center_names.resize(qrydb.start.size() - 1);
    } else {
    std::cout << "Read Centers..." << std::endl;
    }
    if (query_fasta) {
    } else if (LooksLikeFasta(val["center"])) {
      std::vector<hsearch::Kmer> ckmers;
      std::string cerr;
      if (!hsearch::ReadKmerFasta(val["center"], &ckmers)) {
        fprintf(stderr, "cannot open %s\n", val["center"].c_str());
        return EXIT_FAILURE;
      }
      if (!hsearch::CentersFromKmers(ckmers, kmer_length, &center_names, &centers, &cerr, &center_codes)) {
        fprintf(stderr, "ERROR: %s\n", cerr.c_str());
        return EXIT_FAILURE;
      }
    } else if (!hsearch::ReadPointsFile(val["center"], dim, &center_names, &centers)) {
      fprintf(stderr, "cannot open %s\n", val["center"].c_str());
      return EXIT_FAILURE;
    }
    std::vector<double> radii;
    if (with_radii) {
      std::string rerr;
      if (!hsearch::ReadRadiiFile(val["radii"], center_names, &radii, &rerr)) {
        fprintf(stderr, "ERROR: %s\n", rerr.c_str());
        return EXIT_FAILURE;
      }
      // (the evaluation step -g checks a hit's distance against the radius: the largest one here)
      for (double r : radii) hash_R = std::max(hash_R, fabs(r));
    }
    if (!fasta_db) std::cout << "number of kmers " << kmers.size() << std::endl;
    if (query_fasta) std::cout << "number of query proteins " << center_names.size() << std::endl;
    else
    std::cout << "number of centers " << centers.size() << std::endl;
    hsearch::Planes planes;
    if (val.count("planes")) {
      std::string perr;
      if (!hsearch::ReadPlanesFile(val["planes"], dim, hash_K, hash_L, hash_W, &planes, &perr)) {
        fprintf(stderr, "ERROR: %s\n", perr.c_str());
        return EXIT_FAILURE;
      }
    } else {
      planes = hsearch::DrawPlanes(dim, hash_K, hash_L, hash_W, seed);
    }
    const bool use_comm = val.count("gpus") != 0 && !with_radii && !topk;  // (--radii / --topk --gpus 1: the one-GPU path)
    const int n_gpus = use_comm ? atoi(val["gpus"].c_str()) : 1;
    if (n_gpus < 1 || n_gpus > 64) {
      fprintf(stderr, "ERROR: --gpus must be 1..64\n");
      return EXIT_FAILURE;
    }
    const bool by_tables = val.count("partition") && val["partition"] == "tables";
    const bool by_buckets = val.count("partition") && val["partition"] == "buckets";
    if (val.count("partition") && !by_tables && !by_buckets && val["partition"] != "queries") {
      fprintf(stderr, "ERROR: --partition must be queries, tables or buckets\n");
      return EXIT_FAILURE;
    }
    hsearch::SetShardPartition(by_tables ? hsearch::kPartitionTables
                                         : by_buckets ? hsearch::kPartitionBuckets : hsearch::kPartitionQueries);
    const bool loopback = val.count("transport") && val["transport"] == "loopback";
    if (val.count("transport") && !loopback && val["transport"] != "rccl") {
      fprintf(stderr, "ERROR: --transport must be rccl or loopback\n");
      return EXIT_FAILURE;
    }
    if (loopback) hsearch::SetShardTransport(hsearch::kTransportLoopback);
    std::vector<int> devices;
    for (int g = 0; g < n_gpus; ++g) devices.push_back(loopback ? device : device + g);
    if (val.count("planes-out")) {
      std::ofstream pf(val["planes-out"].c_str(), std::ios::binary);
      pf.write(reinterpret_cast<const char*>(planes.a.data()), planes.a.size() * sizeof(double));
      pf.write(reinterpret_cast<const char*>(planes.b.data()), planes.b.size() * sizeof(double));
    }
    if (val.count("planes"))
      printf("hash_K = %u hash_L = %u planes = %s\n", hash_K, hash_L, val["planes"].c_str());
    else
      printf("hash_K = %u hash_L = %u seed = %u\n", hash_K, hash_L, seed);
    if (use_comm && loopback)
      printf("gpus = %d (%d ranks on device %d, hits exchanged through host memory)\n", n_gpus, n_gpus, device);
    else if (use_comm)
      printf("gpus = %d (devices %d..%d, RCCL all-gather of hits)\n", n_gpus, device, device + n_gpus - 1);
    const int probes = val.count("probes") ? atoi(val["probes"].c_str()) : 0;
    if (probes < 0 || probes > 63) {
      fprintf(stderr, "ERROR: --probes must be 0..63\n");
      return EXIT_FAILURE;
    }
    if (probes && fasta_db && !per_sequence) {
      fprintf(stderr, "ERROR: --probes needs a points database\n");
      return EXIT_FAILURE;
    }
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    std::string err;
    std::vector<uint64_t> table_sizes;
    uint64_t n_windows = 0;
    const bool best_per_position = val.count("best-per-position") && atoi(val["best-per-position"].c_str()) != 0;
    const int st =
        per_sequence ? hsearch::SearchProteinsPerSequence(prodb, kmer_length, centers, center_names,
                                                          center_codes.empty() || val.count("centers-as-points")
                                                              ? nullptr : &center_codes,
                                                          query_fasta ? &qrydb : nullptr, hash_K, hash_L, hash_W, hash_R,
                                                          val["output"], planes, device, &err, &table_sizes, &n_windows,
                                                          (uint32_t)probes, with_radii ? &radii : nullptr, &more) :
        fasta_db ? hsearch::SearchProteinsSharded(prodb, kmer_length, centers, center_names, hash_K, hash_L,
                                                  hash_W, hash_R, val["output"], planes, devices, use_comm,
                                                  &err, &table_sizes, &n_windows,
                                                  best_per_position,
                                                  // k-mer centres over a FASTA database share its exact
                                                  // table: they go to the GPU as codes (hs_query_codes)
                                                  center_codes.empty() || val.count("centers-as-points")
                                                      ? nullptr : &center_codes,
                                                  with_radii ? &radii : nullptr, topk, &more)
                 : hsearch::SearchSharded(kmers, centers, kmer_names, center_names, hash_K, hash_L, hash_W,
                                          hash_R, val["output"], planes, devices, use_comm, &err,
                                          &table_sizes, (uint32_t)probes, with_radii ? &radii : nullptr,
                                          best_per_position, topk);
    if (fasta_db && st == 0) std::cout << "number of kmers " << n_windows << std::endl;
    if (st != 0) {
      fprintf(stderr, "ERROR: %s (status %d)\n", err.c_str(), st);
      return EXIT_FAILURE;
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    for (uint64_t ts : table_sizes) std::cout << "table size " << ts << std::endl;
    const double secs = (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
    if (val.count("groundtruth")) {
      std::cout << "evaulate ..." << std::endl;
      printf("ACCURACY: %lf %lf\n", hsearch::Evaluate(val["groundtruth"], val["output"], hash_R), secs);
    } else {
      printf("SEARCH: %lf seconds\n", secs);
    }
  } catch (const std::bad_alloc&) {
    fprintf(stderr, "ERROR: could not allocate memory\n");
    return EXIT_FAILURE;
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
