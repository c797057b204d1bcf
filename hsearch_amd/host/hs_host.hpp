// hs_host.hpp -- C++ host side above the C ABI (include/hsearch.h): the reference's operator
// surface for the search path, with the same names, argument meaning and error behaviour, so a
// caller of acgtun/hsearch's Search() can switch by changing an include and one extra argument
// (the planes, which the reference draws from std::random_device and therefore cannot share).
//
//   reference                                         here
//   struct Point {vector<double> data;}  (:18-23)     hsearch::Point
//   LSH(dim, K, W) x L, random_device    (lsh.hpp)    hsearch::DrawPlanes(dim, K, L, W, seed)
//   Search(kmers, centers, names..., K, L, W, R, out) hsearch::Search(... , planes, device)
//   evaulate(ground_truth, out, R)       (:100-165)   hsearch::Evaluate
//   points-file reader in main()         (:343-370)   hsearch::ReadPointsFile
// (file:line = hclust/src/hclust/motif_both_points.cpp unless noted.)
#ifndef HS_HOST_HPP
#define HS_HOST_HPP

#include <stdint.h>

#include <map>
#include <string>
#include <vector>

struct hs_handle;

namespace hsearch {

struct Point {
  std::vector<double> data;
};
struct Kmer;

// L x K Gaussian normals a ~ N(0,1) (K*dim per table) and offsets b ~ U[0,W), drawn exactly as the
// reference's LSH constructor does (lsh.hpp:10-31: default_random_engine, normal_distribution,
// uniform_real_distribution, per function dim normals then one uniform, fresh distributions per
// table) with the table-l engine seeded by seed + l instead of random_device.
struct Planes {
  uint32_t dim = 0, K = 0, L = 0;
  double W = 0;
  std::vector<double> a;  // [L][K][dim]
  std::vector<double> b;  // [L][K]
};
Planes DrawPlanes(uint32_t dim, uint32_t K, uint32_t L, double W, uint32_t seed);

// The reference's points file: per record one name line and one line of `dim` doubles (:343-354).
bool ReadPointsFile(const std::string& path, uint32_t dim, std::vector<std::string>* names,
                    std::vector<Point>* points);

// DB points -> residue codes + the coordinate table they are embeddings of.  Every 8-tuple of every
// DB point must be one of at most 32 distinct rows (true for anything KmerToCoordinates or
// protein2datapoints produced, including the 6-significant-digit points files).  Returns false
// with *err set when the points are not embeddings of such an alphabet.
bool PointsToCodes(const std::vector<Point>& pts, uint32_t dim, std::vector<double>* table,
                   std::vector<uint8_t>* codes, std::string* err);

// Search() (:195-250).  Builds the L tables over `kmers`, probes them with every centre, verifies
// candidates by squared Euclidean distance <= R*R and writes "<center> <kmer> <dist>" lines in the
// reference's order (centre, table of first sight, ascending k-mer index).  Runs on `device`
// through libhsearch_amd.so; returns 0, or an hs_status with *err set.  table_sizes (optional)
// receives the number of distinct keys per table, which the reference prints (:217).
int Search(const std::vector<Point>& kmers, const std::vector<Point>& centers,
           const std::vector<std::string>& kmer_names, const std::vector<std::string>& center_names,
           const uint32_t& hash_K, const uint32_t& hash_L, const double& hash_W,
           const double& hash_R, const std::string& output_file, const Planes& planes, int device,
           std::string* err, std::vector<uint64_t>* table_sizes = nullptr, uint32_t probes = 0,
           const std::vector<double>* radii = nullptr, bool best_per_position = false, uint32_t topk = 0);
// topk != 0 (Search, SearchProteins and the one-GPU form of their *Sharded() versions): per centre only its topk best
// hits, selected on the device (hs_query_topk in include/hsearch.h) -- the usual lines, per centre at most topk of
// them, in ascending (distance, k-mer index) instead of (table, k-mer index).  It composes with radii and probes; the
// multi-GPU exchange and best_per_position refuse it.
// radii (Search, SearchProteins, SearchBruteForce and the one-GPU form of their *Sharded() versions): one radius
// per centre in place of hash_R -- centre i's lines are those of a run with hash_R = (*radii)[i]
// (hs_query_radii); the multi-GPU exchange takes one radius and refuses them.

// How the rank threads of the *Sharded() functions exchange their hits: RCCL over xGMI (one rank per
// GPU; the default), or host memory between rank threads whose `devices` may repeat -- the whole rank
// protocol (barrier, capacity decision, failed-rank handling) on a box with fewer GPUs than ranks,
// which RCCL refuses (`hs_motif_both_points --transport loopback`).  Process-wide; set before the call.
enum ShardTransport { kTransportRccl = 0, kTransportLoopback = 1 };
void SetShardTransport(ShardTransport t);
// What a rank of the *Sharded() functions holds.  kPartitionQueries (the default): the whole index,
// replicated, and a contiguous block of the centres.  kPartitionTables: a subset of the L tables over ALL
// k-mers (tables dealt to the GPUs by an estimate of their join work, hs_assign_tables) and ALL centres; behind
// the all-gather every rank keeps, per (centre, k-mer), the tuple of the smallest table -- the reference's
// first-seen rule (motif_both_points.cpp:232-238) -- so the file is the same (include/hsearch_dist.h).  A GPU
// then holds and builds 1 / n of the table bytes (configs[2]: 23 GB instead of 157 GB) and every bucket meets
// all centres of the batch at once.  kPartitionBuckets: the whole index, replicated, and ALL centres; the GPUs
// share the BUCKETS (hs_set_bucket_partition: a function of the bucket's key fingerprint, giant buckets shared
// by centre) and the lists are merged by the same rule -- 1 / n of the probes and pairs per GPU, every bucket
// with all the centres there are, even parts whatever the tables look like.  Process-wide; set before the call.
enum ShardPartition { kPartitionQueries = 0, kPartitionTables = 1, kPartitionBuckets = 2 };
void SetShardPartition(ShardPartition p);

// probes (Search, SearchSharded): T extra buckets per table (hs_set_multiprobe, multi-probe LSH); 0 = the
// reference's one probe.  Every partition passes it to every rank's handle.
// Search() spread over the GPUs `devices` of this node: one host thread and one handle
// per GPU, the index replicated (built on every GPU), centre i searched by the rank owning its
// contiguous block (hs_shard_bounds), the hits all-gathered over RCCL (include/hsearch_dist.h) and
// written by rank 0 -- the same file as Search().  use_comm forces the communicator path with a
// single GPU too (`--gpus 1`: RCCL with one rank); Search() is SearchSharded({device}, false).
int SearchSharded(const std::vector<Point>& kmers, const std::vector<Point>& centers,
                  const std::vector<std::string>& kmer_names, const std::vector<std::string>& center_names,
                  const uint32_t& hash_K, const uint32_t& hash_L, const double& hash_W,
                  const double& hash_R, const std::string& output_file, const Planes& planes,
                  const std::vector<int>& devices, bool use_comm, std::string* err,
                  std::vector<uint64_t>* table_sizes = nullptr, uint32_t probes = 0,
                  const std::vector<double>* radii = nullptr, bool best_per_position = false, uint32_t topk = 0);
// best_per_position (Search, SearchSharded; SearchProteins* below): instead of the hits, one line per database
// k-mer reached, "<kmer name> <center> <dist>" with its nearest centre, k-mers ascending -- hs_annotate on one
// GPU; with query blocks over several GPUs every rank annotates its block and the lists are merged by
// hs_merge_best; the table and bucket partitions gather the hits as before and reduce them by hs_merge_best.

// The planes file `--planes-out` writes and `--planes` reads: binary doubles a[L][K][dim], b[L][K].
bool ReadPlanesFile(const std::string& path, uint32_t dim, uint32_t K, uint32_t L, double W, Planes* planes,
                    std::string* err);
// Centres given as k-mers (">name" line, then the k letters -- the k-mer FASTA hclust2.cpp:231-241
// reads) instead of a points file: embedded exactly from the table (KmerToCoordinates,
// hclust2.cpp:49-62).  A letter outside the 20-letter alphabet or another length is an error.
// codes (optional) receives the same centres as rows of the coordinate table, [n][k].
bool CentersFromKmers(const std::vector<Kmer>& kmers, uint32_t kmer_length, std::vector<std::string>* names,
                      std::vector<Point>* centers, std::string* err, std::vector<uint8_t>* codes = nullptr);

// ---- FASTA database: k-mers enumerated on the device ------------------------
// ProteinDB of protein.hpp:41-71: lines starting with '>' are names, every other non-empty line is
// one whole sequence.  Residues are stored as rows of the coordinate table (include/hs_tables.h);
// letters outside the 20-letter alphabet -- the reference substitutes rand() % 20 for them,
// protein.hpp:58-61 -- are stored as kUnknown and no window may contain one.
// ref_compat_eq_swap reproduces the reference's E <-> Q exchange (it stores AA20[base[c]] and later
// embeds base[] of THAT letter, protein.hpp:62 + kmer_search.cpp:56); the default
// is the correct embedding (E -> Glu, Q -> Gln).
struct ProteinDB {
  static const uint8_t kUnknown = 255;
  std::vector<std::string> name;   // '>' lines, without the '>'
  std::vector<uint64_t> start;     // [n_sequences + 1] into residues
  std::vector<uint8_t> residues;   // all sequences, concatenated
  bool eq_swapped = false;
};
bool ReadProteinFasta(const std::string& path, bool ref_compat_eq_swap, ProteinDB* db);

// The search of kmer_search.cpp over a FASTA database, with motif_both_points' verification and
// output: DB = every length-k window (free of unknown letters) of every sequence, enumerated on the
// device by hs_index_build_windows in kmer_search.cpp:64-83 order; hits are written as
// "<center> <kmer name> <dist>" in Search()'s order, a k-mer being named like protein2datapoints
// names its samples (protein2datapoints.cpp:66): <first token of the protein name>#<sequence
// index>$<offset>@<k letters>*<window number>.  n_windows (optional) receives the DB size.
int SearchProteins(const ProteinDB& db, uint32_t kmer_length, const std::vector<Point>& centers,
                   const std::vector<std::string>& center_names, const uint32_t& hash_K,
                   const uint32_t& hash_L, const double& hash_W, const double& hash_R,
                   const std::string& output_file, const Planes& planes, int device, std::string* err,
                   std::vector<uint64_t>* table_sizes = nullptr, uint64_t* n_windows = nullptr,
                   bool best_per_position = false, const std::vector<double>* radii = nullptr, uint32_t topk = 0,
                   const std::vector<ProteinDB>* more = nullptr);
int SearchProteinsSharded(const ProteinDB& db, uint32_t kmer_length, const std::vector<Point>& centers,
                          const std::vector<std::string>& center_names, const uint32_t& hash_K,
                          const uint32_t& hash_L, const double& hash_W, const double& hash_R,
                          const std::string& output_file, const Planes& planes,
                          const std::vector<int>& devices, bool use_comm, std::string* err,
                          std::vector<uint64_t>* table_sizes = nullptr, uint64_t* n_windows = nullptr,
                          bool best_per_position = false, const std::vector<uint8_t>* center_codes = nullptr,
                          const std::vector<double>* radii = nullptr, uint32_t topk = 0,
                          const std::vector<ProteinDB>* more = nullptr);
// more (SearchProteins* all three; one GPU): further databases appended in order -- the index is built over db's windows
// and grown by each of theirs (hs_index_append_windows), sequence numbers and names continue; the output is that of
// one database holding all the sequences.
// The per_sequence mode of SearchProteins: instead of the hits, one line per (centre, database protein) with a hit,
// reduced on the device (hs_seq_match in include/hsearch.h; the hit list never reaches the host) --
//   <centre name> <protein>#<its number> <hits> <offset of the best window> <its distance> <first> <last matched offset>
// rows ascending in (centre, protein), offsets in residues of the protein, the distance printed with %.17g.  query
// != nullptr: the queries are every length-k window of the proteins of `query` (centers, center_names and
// center_codes unused), the groups are the query proteins and diagonals are kept: one line per (query protein,
// database protein, diagonal), named <query protein>#<its number>, the best offset that of the database window, the
// diagonal (database window number in its protein minus query offset) as the last field.  A protein with letters
// outside the alphabet has no window across them; its window numbers, which the diagonal is made of, then run
// behind its residue offsets.  radii: one per centre, or per query protein.  probes: multi-probe, as in Search().
// One GPU.
int SearchProteinsPerSequence(const ProteinDB& db, uint32_t kmer_length, const std::vector<Point>& centers,
                              const std::vector<std::string>& center_names, const std::vector<uint8_t>* center_codes,
                              const ProteinDB* query, const uint32_t& hash_K, const uint32_t& hash_L,
                              const double& hash_W, const double& hash_R, const std::string& output_file,
                              const Planes& planes, int device, std::string* err,
                              std::vector<uint64_t>* table_sizes = nullptr, uint64_t* n_windows = nullptr,
                              uint32_t probes = 0, const std::vector<double>* radii = nullptr,
                              const std::vector<ProteinDB>* more = nullptr);
// `--pssm FILE`: position-specific score matrices over a FASTA database (hs_pssm_scan: every window of every protein
// scored, exhaustively; no hash tables take part).  The file: per profile a line ">name threshold", then kmer_length
// lines of 20 numbers, the columns in the coordinate table's residue order (HS_CODE_TO_LETTER).  A profile with
// another shape, a number that is none, a name without a threshold or a name given twice is an error (*err).
// S [nm][kmer_length][20], t [nm].
bool ReadPssmFile(const std::string& path, uint32_t kmer_length, std::vector<std::string>* names,
                  std::vector<double>* S, std::vector<double>* t, std::string* err);
// The scan: one line per hit, "<profile name> <window name> <score>" with the window named as SearchProteins names
// it and the score printed with 17 significant digits (it reads back bit for bit), in (profile, window) order.
// Windows never cross a letter outside the alphabet.  One GPU.
int ScanProfiles(const ProteinDB& db, uint32_t kmer_length, const std::vector<std::string>& names,
                 const std::vector<double>& S, const std::vector<double>& t, const std::string& output_file,
                 int device, std::string* err, uint64_t* n_windows = nullptr, uint64_t* n_hits = nullptr);
// `--pssm FILE --pssm-top N`: per profile at most N lines, its N best windows among those scoring at or above the
// file's threshold (the floor), selected on the device (hs_pssm_topk; 1 <= N <= 64).  The same lines as ScanProfiles
// writes; profiles in file order, within a profile by descending score, then ascending window index.
int ScanProfilesTopN(const ProteinDB& db, uint32_t kmer_length, const std::vector<std::string>& names,
                     const std::vector<double>& S, const std::vector<double>& t_floor, uint32_t topn,
                     const std::string& output_file, int device, std::string* err, uint64_t* n_windows = nullptr,
                     uint64_t* n_lines = nullptr);
// `--pssm FILE --pssm-per-sequence 1`: one line per (profile, protein) with a hit, reduced on the device
// (hs_pssm_seq_scan): "<profile name> <protein>#<number> <hits> <offset of the best window> <its score> <first> <last
// matched offset>", the offsets in residues from the protein's start, the score with 17 significant digits; profiles
// in file order, proteins in database order.  *n_hits: the hits behind the rows, *n_rows: the lines.
int ScanProfilesPerSequence(const ProteinDB& db, uint32_t kmer_length, const std::vector<std::string>& names,
                            const std::vector<double>& S, const std::vector<double>& t, const std::string& output_file,
                            int device, std::string* err, uint64_t* n_windows = nullptr, uint64_t* n_hits = nullptr,
                            uint64_t* n_rows = nullptr);
// The file ReadPssmFile reads, every number printed as %.17g: it reads back bit for bit.
bool WritePssmFile(const std::string& path, uint32_t kmer_length, const std::vector<std::string>& names,
                   const std::vector<double>& S, const std::vector<double>& t, std::string* err);
// `--pssm FILE --pssm-refine N`: the profiles rebuilt from their own hits over the database's windows (hs_pssm_refine:
// scan, counts, log-odds against the database's residue composition, at most n_iter scans at the fixed thresholds t).
// one_per_protein: only the best window of every protein counts.  S_out: the refined profiles.  One GPU.
int RefineProfiles(const ProteinDB& db, uint32_t kmer_length, const std::vector<double>& S, const std::vector<double>& t,
                   uint32_t n_iter, bool one_per_protein, double pseudo, int device, std::vector<double>* S_out,
                   uint32_t* iters, bool* converged, std::string* err);
// `--pssm FILE --pssm-rank N`: per profile the score of its rank-th best window over the database (hs_pssm_rank) -- the
// threshold at which a scan returns the rank best windows and their ties.  rank [nm], each 1 .. the number of windows
// (*n_windows; a rank outside is HS_ERR_INVALID).  t_out [nm]; cnt_ge (may be null): the windows at or above it.  One GPU.
int RankThresholds(const ProteinDB& db, uint32_t kmer_length, const std::vector<double>& S,
                   const std::vector<uint64_t>& rank, int device, std::vector<double>* t_out,
                   std::vector<uint64_t>* cnt_ge, uint64_t* n_windows, std::string* err);
// `--pssm FILE --pssm-rank N --pssm-refine I`: RefineProfiles with the threshold rule (hs_pssm_refine_rank): every scan
// runs at the threshold that admits the rank[m] best windows of the current matrix.  t_out: the last scan's thresholds.
int RefineProfiles(const ProteinDB& db, uint32_t kmer_length, const std::vector<double>& S,
                   const std::vector<uint64_t>& rank, uint32_t n_iter, bool one_per_protein, double pseudo, int device,
                   std::vector<double>* S_out, std::vector<double>* t_out, uint32_t* iters, bool* converged,
                   std::string* err);
// `--pssm FILE --pssm-refine N --pssm-weights sites|columns`: RefineProfiles on Henikoff-weighted counts
// (hs_pssm_refine_weighted).  Exactly one of t (fixed thresholds) and rank (the threshold rule; t_out is required then)
// is given.  neff_columns: the log-odds take n_eff = distinct / k, else n_eff = the sites.
int RefineProfilesWeighted(const ProteinDB& db, uint32_t kmer_length, const std::vector<double>& S,
                           const std::vector<double>* t, const std::vector<uint64_t>* rank, bool neff_columns,
                           uint32_t n_iter, bool one_per_protein, double pseudo, int device, std::vector<double>* S_out,
                           std::vector<double>* t_out, uint32_t* iters, bool* converged, std::string* err);
// `--pssm FILE --pssm-pvalue P`: per profile the threshold of the p-value p[m] in (0, 1] under the null model of the
// database's residue composition (hs_pssm_pvalue_threshold with bg = NULL), on a score grid from t_lo[m] to the
// profile's maximal score.  t_out [nm]; p_hi, p_lo (may be null): the bracket of the p-value at t_out; flag (may be
// null): 0 exact on the grid, 1 clipped at t_lo, 2 nothing admissible (t_out = +DBL_MAX: a scan finds nothing).  One GPU.
int PvalueThresholds(const ProteinDB& db, uint32_t kmer_length, const std::vector<double>& S,
                     const std::vector<double>& p, const std::vector<double>& t_lo, int device,
                     std::vector<double>* t_out, std::vector<double>* p_hi, std::vector<double>* p_lo,
                     std::vector<uint32_t>* flag, std::string* err);
// `--pssm FILE --pssm-compare FILE2|self`: profile against profile at every offset (hs_pssm_compare; no database, no
// index).  X [nx][kmer_length][20] with names_x and thresholds t [nx]; Y / names_y null: X against itself (pairs
// x < y).  columns: 0 Pearson, 1 cosine (hs_pssm_compare_columns applied to both sides first), -1 raw.  One line per
// hit, "<nameX> <nameY> <d> <score>", the score with 17 significant digits, in (x, y) order.  One GPU.
int CompareProfiles(uint32_t kmer_length, const std::vector<std::string>& names_x, const std::vector<double>& X,
                    const std::vector<double>& t, const std::vector<std::string>* names_y, const std::vector<double>* Y,
                    uint32_t min_overlap, int columns, const std::string& output_file, int device, std::string* err,
                    uint64_t* n_hits = nullptr, const std::string* families_out = nullptr,
                    uint64_t* n_families = nullptr, uint64_t* n_conflicts = nullptr);
// (families_out, self mode only: the hits are also laid out as families as FamilyLayout does and written to that
// file; the layout is computed before either file is written, so a refused layout leaves no output behind)
// `--pssm-compare self --pssm-families-out FAM`: the hits of a self comparison, in their order, to families
// (hs_pssm_family_layout): FAM gets one line per profile, "<family> <profile name> <offset>", in the order in which to
// pass the profiles to FamilyScan -- by (family, offset, profile) --, the family named after its first profile in that
// order.  *n_conflicts: the hits that disagreed with the positions fixed before them.  Host only.
int FamilyLayout(const std::vector<std::string>& names, const std::vector<uint32_t>& hit_x,
                 const std::vector<uint32_t>& hit_y, const std::vector<int32_t>& hit_d, const std::string& families_file,
                 std::string* err, uint64_t* n_families = nullptr, uint64_t* n_conflicts = nullptr);
// `--pssm FILE --pssm-families FAM`: the hits of the profiles reduced per (family, protein, diagonal) on the device
// (hs_pssm_family_scan).  family [nm], offset [nm]: every profile's family name and offset in it; the profiles of one
// family stand next to each other (HS_ERR_INVALID otherwise).  A row is written when at least min_blocks profiles hit
// on the diagonal and (threshold given) their scores add up to *threshold.  One line per row, "<family> <protein>#<number>
// <diag> <blocks> <sum> <best profile> <offset of the best window> <its score> <first> <last matched offset>": diag in
// windows, the offsets in residues from the protein's start, sum and score with 17 significant digits; families in the
// given order, proteins in database order.  *n_hits: the hits behind the rows, *n_rows: the lines.  One GPU.
int FamilyScan(const ProteinDB& db, uint32_t kmer_length, const std::vector<std::string>& names,
               const std::vector<double>& S, const std::vector<double>& t, const std::vector<std::string>& family,
               const std::vector<uint32_t>& offset, uint32_t min_blocks, const double* threshold,
               const std::string& output_file, int device, std::string* err, uint64_t* n_windows = nullptr,
               uint64_t* n_hits = nullptr, uint64_t* n_rows = nullptr);
// `--pssm FILE --pssm-families FAM --pssm-family-shift G`: per (family, protein) the best gapped chain of the family's
// hits on the device (hs_pssm_family_chain): hits of later profiles at later offsets link when their diagonals differ by
// at most max_shift, at the cost gap_open + gap_ext * d for d >= 1.  family, offset: as for FamilyScan, and the offsets
// must not decrease inside a family (HS_ERR_INVALID otherwise).  A chain is written when it holds at least min_blocks
// hits and (threshold given) scores at least *threshold.  One line per chain, "<family> <protein>#<number> <blocks>
// <gaps> <score> <first profile> <first offset> <last profile> <last offset> <shift>": the offsets in residues from the
// protein's start, the score with 17 significant digits, shift = the last hit's diagonal minus the first's; families in
// the given order, proteins in database order.  *n_hits: the hits behind the chains, *n_rows: the lines.  One GPU.
int FamilyChain(const ProteinDB& db, uint32_t kmer_length, const std::vector<std::string>& names,
                const std::vector<double>& S, const std::vector<double>& t, const std::vector<std::string>& family,
                const std::vector<uint32_t>& offset, uint32_t max_shift, double gap_open, double gap_ext,
                uint32_t min_blocks, const double* threshold, const std::string& output_file, int device,
                std::string* err, uint64_t* n_windows = nullptr, uint64_t* n_hits = nullptr, uint64_t* n_rows = nullptr);
// `--pssm FILE --pssm-pvalue-column 1`: ScanProfiles' lines with " <p_hi>" appended, the upper end of the hit's p-value
// under the same null model (hs_pssm_pvalue), printed with 17 significant digits; t_lo [nm]: the grids' floors.
int HitPvalues(const ProteinDB& db, uint32_t kmer_length, const std::vector<std::string>& names,
               const std::vector<double>& S, const std::vector<double>& t, const std::vector<double>& t_lo,
               const std::string& output_file, int device, std::string* err, uint64_t* n_windows = nullptr,
               uint64_t* n_hits = nullptr);
// center_codes (CentersFromKmers): the centres are k-mers of the exact table -- the one a FASTA
// database is embedded from -- and travel to the GPU as residue codes (hs_query_codes: k bytes per
// centre instead of 64 k); the hits are those of the embedded centres, bit for bit.
// best_per_position: what kmer_search.cpp's Search() accumulates in `matches` (:90,113-121) and
// never writes -- for every database window with a hit, its nearest centre: tables ascending,
// centres ascending within a table, replaced only by a strictly smaller distance.  Written as
// "<kmer name> <center> <dist>", windows ascending.  (The reference's own result is not
// observable and is computed from mis-hashed windows, kmer_search.cpp:73-80 reads one residue k
// times; this is the intended reduction over the pinned hit list -- parity unpinned.)

// Protein2Datapoints() (protein2datapoints.cpp:33-78): the sampler that makes the `-d` points file
// of motif_both_points from a FASTA database -- for each of the first num_of_protein_out
// sequences, windows at offsets 0, then +30..49 (30 + rand() % 20) further each time; a window seen
// before is skipped (same stride draw); each new one is written as the name line
// "<first token of the protein name>#<sequence>$<offset>@<letters>*<count>" and the embedding at
// the stream's default precision.  rand() is seeded with `seed` (the reference: time(NULL)).
// Sequences shorter than k are skipped (the reference's unsigned `length - k` wraps, :44) and so
// are windows with a letter outside the alphabet (the reference draws a random residue instead,
// protein.hpp:58-61).  Returns the number of points written, -1 if the file cannot be written.
int64_t Protein2Datapoints(const ProteinDB& db, uint32_t kmer_length, uint32_t num_of_protein_out,
                           const std::string& output_file, uint32_t seed);

// ---- Kernel-LSH pre-grouping of whole proteins (pcluster.cpp:11-81) ---------
// pcluster's FASTA reader (read_proteins.cpp:6-41): '>' lines start a protein, its name is the
// text up to the first space, the following lines are concatenated; letters of the 20-letter
// alphabet are kept, any other alphabetic character is replaced by a residue drawn from a
// generator seeded with unknown_seed (the reference uses rand() % 20, read_proteins.cpp:30-32),
// everything else is dropped.
struct PclusterDB {
  std::vector<std::string> names, seqs;
};
bool ReadPclusterFasta(const std::string& path, uint32_t unknown_seed, PclusterDB* db);
// PreClustering(proteinDB, hash_buckets): KLSH(8^3, 16, 0.2) codes of all proteins with at least 3
// residues, computed on `device` (hs_klsh_codes), grouped: buckets[code] = ascending protein
// indices.  Returns 0 or an hs_status with *err set.
int PreClustering(const PclusterDB& db, int device,
                  std::map<uint64_t, std::vector<uint32_t> >* hash_buckets, std::string* err);

// Clustering() of hclust2.cpp:86-151.  kmers: name + sequence (letters of the 20-letter alphabet; a
// letter outside it is replaced by a residue drawn from a generator seeded with `unknown_seed`,
// where the reference uses rand()%20, hclust2.cpp:54-56).  Writes the reference's clusters file
// ("#clusterid:<i>:size<m>" + member names, :137-150).  Returns 0 or an hs_status with *err set.
struct Kmer {
  std::string name, seq;
};
// hclust2's reader (:231-241): whitespace tokens, ">name" then the sequence token.
bool ReadKmerFasta(const std::string& path, std::vector<Kmer>* kmers);
int Clustering(const std::vector<Kmer>& kmers, const uint32_t& hash_K, const uint32_t& hash_L,
               const double& hash_W, const double& hash_R, const std::string& output_file,
               const Planes& planes, int device, uint32_t unknown_seed, std::string* err,
               uint64_t* n_clusters = nullptr);
// What ClusterProfiles writes (below); min_size == 0: no profiles.  Components, SingleLinkageTree, Dbscan and DensityTree
// take a pointer to one (null: none) and then call ClusterProfiles on the labels they just found.
struct ClusterProfileOptions {
  uint32_t min_size = 0;  // members a cluster needs to get a profile
  int weights = 1;        // 0 none (raw counts), 1 sites (n_eff = the members), 2 columns (n_eff = distinct / k)
  int threshold = 0;      // 0 cover (hs_cluster_pssm_cover's min_score), 1 rank (hs_pssm_rank at rank = the members)
  double pseudo = 1.0;    // pseudo-counts of the log-odds, finite and > 0
};
// Single linkage at radius R in place of the greedy leader pass: the clusters are the connected components of
// the graph of all k-mer pairs that share a bucket in one of the L tables and lie within R (sqrt(d2) <= R, the
// test of hclust2.cpp:64-71), which do not depend on the order of the k-mers.  One handle with all L tables, one
// index build, one hs_components: no edge list anywhere.  The same clusters-file format, clusters in ascending
// smallest member, members in ascending index; a k-mer without a neighbour is a cluster of size 1.
int Components(const std::vector<Kmer>& kmers, const uint32_t& hash_K, const uint32_t& hash_L, const double& hash_W,
               const double& hash_R, const std::string& output_file, const Planes& planes, int device,
               std::string* err, uint64_t* n_clusters = nullptr, uint32_t unknown_seed = 0,
               uint32_t centers_min_size = 0, const ClusterProfileOptions* profiles = nullptr);
// Components, and beside the clusters file the single-linkage tree up to R (hs_msf in include/hsearch.h: the minimum
// spanning forest of the same graph under the order (distance, smaller index, larger index)) as
// <output_file>hclust.tree.txt: one line per tree edge in merge order, "<name> <name> <distance>" -- the k-mer with
// the smaller index first, the distance with 17 significant digits, so that it reads back bit for bit.  Cutting the
// list after its first n - c lines gives c clusters; the lines with a distance <= r give the clusters at radius r.
// The clusters file is the one Components writes (the labels are hs_msf's, equal to hs_components').
int SingleLinkageTree(const std::vector<Kmer>& kmers, const uint32_t& hash_K, const uint32_t& hash_L,
                      const double& hash_W, const double& hash_R, const std::string& output_file, const Planes& planes,
                      int device, std::string* err, uint64_t* n_clusters = nullptr, uint64_t* n_tree_edges = nullptr,
                      uint32_t unknown_seed = 0, uint32_t centers_min_size = 0,
                      const ClusterProfileOptions* profiles = nullptr);
// Density clusters (DBSCAN, hs_dbscan in include/hsearch.h) of the same graph: only k-mers with at least min_pts
// neighbours within R (themselves counted) join clusters together, so that one stray k-mer between two families no
// longer fuses them; a sparse k-mer goes to the cluster of its dense neighbour with the smallest index or is noise.
// The format of Components: clusters in ascending label (a cluster's label is its smallest dense member), members
// in ascending index; then, only if there is noise, one block "#noise:size<N>" with the noise k-mers' names in
// ascending index.  *n_clusters does not count that block.
int Dbscan(const std::vector<Kmer>& kmers, const uint32_t& hash_K, const uint32_t& hash_L, const double& hash_W,
           const double& hash_R, const uint32_t& min_pts, const std::string& output_file, const Planes& planes, int device,
           std::string* err, uint64_t* n_clusters = nullptr, uint32_t unknown_seed = 0, uint32_t centers_min_size = 0,
           const ClusterProfileOptions* profiles = nullptr);
// The density tree (hs_density_tree in include/hsearch.h: DBSCAN at every radius up to R) of the same graph at min_pts.
// The clusters file, in Dbscan's format, holds the DBSCAN* clusters at R: Dbscan's with their border k-mers moved to
// the noise block.  <output_file>hclust.core.txt always: one line per k-mer, "<name> <core distance>", "inf" for none.
// With tree, <output_file>hclust.tree.txt in SingleLinkageTree's format: one line per merge in merge order, the
// mutual-reachability weight as the distance.  Numbers with 17 significant digits: they read back bit for bit.
int DensityTree(const std::vector<Kmer>& kmers, const uint32_t& hash_K, const uint32_t& hash_L, const double& hash_W,
                const double& hash_R, const uint32_t& min_pts, const std::string& output_file, const Planes& planes,
                int device, std::string* err, bool tree = false, uint64_t* n_clusters = nullptr,
                uint64_t* n_tree_edges = nullptr, uint32_t unknown_seed = 0, uint32_t centers_min_size = 0,
                const ClusterProfileOptions* profiles = nullptr);
// The k-nearest-neighbour graph within R of the same k-mers (hs_self_knn in include/hsearch.h; hclust2's test
// sqrt(d2) <= R) as <output_file>hclust.knn.txt: one line per k-mer in input order, "<name> <degree>" and then, for its
// min(topk, degree) nearest neighbours in ascending (distance, index), " <neighbour name> <distance>".  The degree is
// the full number of neighbours within R; distances with 17 significant digits, so that they read back bit for bit.
// It opens a handle and builds an index of its own.  Returns 0 or an hs_status with *err set.
int KnnGraph(const std::vector<Kmer>& kmers, const uint32_t& hash_K, const uint32_t& hash_L, const double& hash_W,
             const double& hash_R, const uint32_t& topk, const std::string& output_file, const Planes& planes, int device,
             std::string* err, uint64_t* n_edges = nullptr, uint32_t unknown_seed = 0);
// centers_min_size != 0 (Components, Dbscan, DensityTree): beside the clusters file, ClusterCenters() of the labels just found.
// From cluster labels to the `-c` / `--radii` inputs of motif_both_points, on the handle that holds the k-mers'
// index: label [n] as hs_components / hs_dbscan return it (HS_NOISE or a value < n).  Per cluster of at least min_size
// members, in ascending label, <output_file>hclust.format.txt receives its centroid (hs_cluster_profile) in
// Cluster2DataPoint's format -- the name line is "<name of k-mer `label`>:size<members>" (ReadKmerFasta's names are
// whitespace-free tokens, so the line holds no space and "<name> <radius>" splits at its only one) -- and
// <output_file>hclust.radii.txt "<that name> <radius>" with 17 significant digits.  The radii are taken as FamilyRadii
// takes them: against the centroids AS WRITTEN and read back (hs_cluster_radii with the read-back points), so that a
// search given both files reports every member of every cluster.  Returns 0 or an hs_status with *err set.
int ClusterCenters(hs_handle* h, const std::vector<Kmer>& kmers, const std::vector<uint32_t>& label, uint32_t min_size,
                   const std::string& output_file, std::string* err, uint64_t* n_centers = nullptr);
// From cluster labels to the `--pssm` input of motif_both_points, on the handle that holds the k-mers' index: per
// cluster of at least opt.min_size members, in ascending label, <output_file>hclust.pssm.txt receives a profile named
// as ClusterCenters names the centre, through WritePssmFile (it reads back bit for bit).  The profile: the log-odds
// (hs_pssm_log_odds_weighted of hs_cluster_weighted_profile's position-based sequence weights; with weights == 0
// hs_pssm_log_odds of the raw counts) against hs_pssm_background of the composition of all n k-mers, pseudo-counts
// opt.pseudo.  Its threshold: the covering threshold (hs_cluster_pssm_cover: the scan reports every member of the
// cluster under its profile) or the score of its size-th best k-mer (hs_pssm_rank).  Returns 0 or an hs_status with
// *err set.
int ClusterProfiles(hs_handle* h, const std::vector<Kmer>& kmers, const std::vector<uint32_t>& label,
                    const ClusterProfileOptions& opt, const std::string& output_file, std::string* err,
                    uint64_t* n_profiles = nullptr);

// evaulate() (:100-165) with weight() (:67-87): weighted recall of a hits file against a ground
// truth file sorted by (motif, protein); also writes <output_file>.accuracy.txt.  Returns NaN
// where the reference would exit(0) on an inconsistent ground truth (:68-71).
double Evaluate(const std::string& ground_truth, const std::string& output_file, const double& hash_R);

// ---- brute force (row a11) ----------------------------------------------------------------------
// Search() of motif_both_points_noLSH.cpp:36-56: every (centre, k-mer) pair, centre-major, k-mer
// ascending; "<center> <kmer> <dist>" to output_file unless sqrt(d2) > R.  The reference also
// writes every excluded pair to <output_file>notlessthan.txt (:41-49, Q x N lines); here only when
// write_not_less_than is set.  Distances come from hs_bruteforce (exact fp64, reference order).
int SearchBruteForce(const std::vector<Point>& kmers, const std::vector<Point>& centers,
                     const std::vector<std::string>& kmer_names,
                     const std::vector<std::string>& center_names, const double& hash_R,
                     const std::string& output_file, int device, std::string* err,
                     bool write_not_less_than = false, const std::vector<double>* radii = nullptr);

// The radii file of `--radii`: lines "<centre name> <radius>", any order, matched by name against the centres.
// A centre without a line, a name given twice, a name that is no centre's or a radius that is not one finite
// number is an error (*err says which).  radii[i] belongs to center_names[i].
bool ReadRadiiFile(const std::string& path, const std::vector<std::string>& center_names,
                   std::vector<double>* radii, std::string* err);
// The per-family radius hs_center_distance_sampling writes: the smallest double R with R * R >= d2 (the hit
// rule squares R).
double RadiusCovering(double d2);

// ---- evaluation tooling ------------------------------------------------------
// evaluate2.cpp as it runs (:73-95): the hits file sorted by (motif, protein) and written
// tab-separated to <hits_file>sort.txt -- the ground-truth form evaulate()/Evaluate() expects.
bool SortHitsFile(const std::string& hits_file, uint64_t* n_records = nullptr);
// evaluate2.cpp's comparison (:98-153, unreachable in the reference behind the early return :95):
// weighted recall of hits_file against the ground truth with weight() of :62-71 (49.38 form).
// ground_truth is sorted here as main() does (:88); returns tp / (tp + fn).
double Evaluate2(const std::string& ground_truth, const std::string& hits_file, double* tp = nullptr,
                 double* fn = nullptr);

// ---- motif families -> centroid queries (centerDistanceSmapling.cpp) ---------------------------
// The motif-family file read by main() (:436-456): a line starting with '#' opens a family (the
// whole line is its name), every other non-empty line is one member k-mer; families with fewer
// than min_size members are dropped (MIN_SIZE_CLUSTER = 50, :12).
struct MotifFamily {
  std::string name;
  std::vector<std::string> seqs;
};
bool ReadMotifFamilies(const std::string& path, uint32_t min_size, std::vector<MotifFamily>* families);
// Center() (:67-78) of the members' embeddings (KmerToCoordinates :41-56): coordinate sums in
// member order, then one division by the member count.  A letter outside the 20-letter alphabet --
// the reference substitutes rand() % 20 (:47-49) -- or a member of another length is an error.
bool FamilyCenters(const std::vector<MotifFamily>& families, uint32_t kmer_length,
                   std::vector<Point>* centers, std::string* err);
// cluster2datapoint() (:110-136): the centres as a points file <output_file>hclust.format.txt
// (family name line, then the coordinates), i.e. the `-c` input of motif_both_points.
bool Cluster2DataPoint(const std::vector<MotifFamily>& families, const std::vector<Point>& centers,
                       const std::string& output_file);
// Beside it <output_file>hclust.radii.txt, "<family name> <radius>" per family (the `--radii` input of
// motif_both_points): the radius that makes the family's members hits of its own centroid -- the reference's
// cluster.radius (hclust.cpp:217-222, the largest member-to-centre distance) taken against the centroid AS
// WRITTEN to hclust.format.txt (read back: it is printed at 6 significant digits), d2 summed left to right like
// PairwiseDistance_square, R = RadiusCovering(d2), printed with 17 significant digits.  quantile in (0, 1]: the
// nearest-rank quantile of the members' d2 in place of the maximum (1).  Call after Cluster2DataPoint.
bool FamilyRadii(const std::vector<MotifFamily>& families, uint32_t kmer_length, const std::string& output_file,
                 double quantile, std::string* err);
// sequencedatabase2centers() (:138-190), the function main() runs: all centre-to-centre distances
// (i < j) to <dir>/<output_file>innercenter_protein_centers_0.txt, and the distance of each of
// the first min(100000, N) database points to each centre (centre-major) to
// <dir>/<output_file>ramdom_protein_centers_0.txt.  The reference hard-codes dir =
// "./pro2centerdis" (which must exist) and reads 100000 points whatever N is; here dir is created
// if missing.  The N x C distances are computed on `device` (hs_bruteforce).
int SequenceDatabase2Centers(const std::vector<Point>& kmers_proteins,
                             const std::vector<Point>& centers, const std::string& output_file,
                             const std::string& dir, int device, std::string* err);

}  // namespace hsearch

#endif
