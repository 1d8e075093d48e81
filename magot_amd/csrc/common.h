// Internal definitions shared by the libmagot translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/magot.h"
#include "hostutil.h"
#include "textindex.h"

namespace magot {

// ---------------------------------------------------------------------------
// Genome layout in HBM
// ---------------------------------------------------------------------------
// All contigs live in one global base coordinate space.  Coordinate 0 is
// preceded by kOrigin pad bases so that a 16-base window ending at any real
// base never starts below 0 (the reverse-strand gather reads [hi-15, hi]).
constexpr uint64_t kOrigin = 64;
// Exception-run directory granularity: one u32 per 4096 bases.
constexpr int kDirShift = 12;
constexpr uint32_t kDirClean = 0x80000000u;  // no run touches this block
constexpr uint64_t kRcBit = 1ull << 63;

// A maximal run of one byte that is not in ACGTacgt (N, n, IUPAC, '-', ' ' ...).
struct ExcRun {
  uint64_t start;  // global coordinate of the first base
  uint32_t len;
  uint32_t byte;   // the raw byte
};
static_assert(sizeof(ExcRun) == 16, "ExcRun must be 16 bytes");

struct HostPacked {
  // Forward nibble plane over [0, span) bases (span: multiple of 32 with >= 64
  // bases of zero padding past the last contig).  Base g is nibble g & 7 of
  // word g >> 3: bits 0-1 code (A C G T = 0..3), bit 2 soft-masked
  // (lower-case), bit 3 exception (byte kept in `runs`, code bits 0).  The
  // device mirrors it into the reverse-strand plane (mirror_planes).
  // Every word is written by the packer (no zero-fill pass).
  std::unique_ptr<uint32_t[]> nib;
  uint64_t nib_words = 0;
  uint64_t span = 0;
  std::vector<ExcRun> runs;       // sorted by start, sentinel appended
  std::vector<uint32_t> dir;      // per 4096-block first run with end > block start
  std::vector<uint64_t> contig_base;
  std::vector<uint64_t> contig_len;
  uint64_t extent = 0;            // first coordinate past the last contig
};

// A contig's bytes: contiguous (width == 0: ptr[0, len)), or still in FASTA
// line layout -- every line `width` sequence bytes then a `term`-byte line
// terminator, the last line holding the remainder -- so the packer reads
// the file text directly.
struct ContigSource {
  const uint8_t* ptr;
  uint64_t len;    // bases
  uint64_t width;  // 0: contiguous
  uint32_t term;   // 1 ("\n") or 2 ("\r\n")
};

// FASTA text -> contigs with GenomeSequence semantics (fasta.cpp).  Records
// whose lines are not uniform are stripped into `storage`.  Returns
// MAGOT_ERR_UNSUPPORTED for headers only the Python reader handles exactly.
struct FastaContigs {
  std::vector<std::string> names;
  std::vector<ContigSource> src;
  std::vector<std::string> storage;
};
int scan_fasta(const char* text, uint64_t n, bool truncate, FastaContigs* out);
// The contig's bases, contiguous, into dst[0, src.len).
void copy_contig(const ContigSource& src, uint8_t* dst);

// Packs contig bytes (multi-threaded host code, pack.cpp).
void pack_genome(const ContigSource* src, uint32_t n, HostPacked* out);
// The coordinate layout alone (contig bases, extent, span, nib_words).
void pack_layout(const ContigSource* src, uint32_t n, HostPacked* out);
// out->dir from out->runs (sorted, sentinel appended) and out->extent.
void exc_runs_directory(HostPacked* out);
// bases [pos, pos + n) of a contig, contiguous, into dst (fasta.cpp).
void copy_bases(const ContigSource& src, uint64_t pos, uint64_t n, uint8_t* dst);

// Device packing (devpack.hip): raw = the contigs' bytes concatenated in
// coordinate order (raw index i = global base kOrigin + i), n bytes, padded
// with readable bytes to a multiple of 32.
size_t devpack_scan_bytes(uint64_t n_groups);
// count[g] = exception runs starting in raw bytes [32g, 32g+32); slot = their
// exclusive prefix sum (n_groups = ceil(n / 32) entries each).
hipError_t launch_run_count(const uint8_t* raw, uint64_t n, uint32_t* count, uint64_t* slot,
                            void* scan_tmp, size_t scan_bytes, hipStream_t s);
// every run's first coordinate, end coordinate (exclusive) and byte, in order
void launch_run_write(const uint8_t* raw, uint64_t n, const uint64_t* slot, uint64_t* run_start,
                      uint64_t* run_end, uint8_t* run_byte, hipStream_t s);
// the forward nibble plane, nib_words words (pad bases 0)
void launch_nib_pack(const uint8_t* raw, uint64_t n, uint32_t* nib, uint64_t nib_words,
                     hipStream_t s);
// dst[dst_off[i], dst_off[i+1]) = src[src_off[i], ...) for i < n (devpack.hip)
void launch_segments_copy(const uint8_t* src, const uint64_t* src_off, const uint64_t* dst_off,
                          uint64_t n, uint8_t* dst, hipStream_t s);

// Compact replica image of a packed genome (wire.hip; magot_genome_wire_*).
constexpr uint64_t kWireMagic = 0x3257544f47414d00ull;  // "\0MAGOTW2"
struct WireHeader {
  uint64_t magic;
  uint64_t span;       // of the genome it was cut from
  uint64_t n_mask;     // soft-mask runs (the sentinel pair follows them)
  uint64_t n_mdir;     // mask directory entries
  uint64_t o_code2, o_mask, o_mdir, o_exc;  // byte offsets in the image
  uint64_t exc_bytes;  // the arena's exception runs + directory region
  uint64_t total;      // image bytes
  uint64_t meta_hash;  // FNV-1a of the genome's meta blob (magot_genome_export)
};
size_t wire_scan_bytes(uint64_t groups);
// count[g] = soft-mask runs starting in bases [32g, 32g+32) of the forward
// plane; slot = their exclusive prefix sum (span / 32 entries each)
hipError_t launch_wire_count(const uint32_t* nib, uint64_t span, uint32_t* count, uint64_t* slot,
                             void* scan_tmp, size_t scan_bytes, hipStream_t s);
// every mask run's {start, end} at its slot (u32 pairs)
void launch_wire_runs(const uint32_t* nib, uint64_t span, const uint64_t* slot, uint32_t* runs,
                      hipStream_t s);
void launch_wire_mdir(const uint32_t* runs, uint64_t n, uint64_t n_blocks, uint32_t* mdir,
                      hipStream_t s);
// the forward nibble plane (span / 8 words) from an image's pieces
void launch_wire_unpack(const uint32_t* code2, const uint32_t* mask, uint64_t n_mask,
                        const uint32_t* mdir, uint64_t n_mdir, const ExcRun* exc, uint64_t n_exc,
                        const uint32_t* edir, uint64_t n_edir, uint64_t span, uint32_t* nib,
                        hipStream_t s);

// ---------------------------------------------------------------------------
// Extraction tiling
// ---------------------------------------------------------------------------
constexpr int kThreads = 256;                 // one workgroup = 4 independent waves
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 16;                    // bytes per lane-store
// Chunk slots per lane per tile: 6 (6096-byte tiles) for large plans; 3
// (3024-byte tiles) for translating plans too small to fill the chip several
// times over (one GPU's share of an 8-GPU C4 job: -3.5 % per launch; 4-GPU
// share -2.7 %; but the 2-GPU share +8 %, C2 (nucleotides only) +5.5 %;
// EXPERIMENTS.md §3).  Full C3: 6 slots -2.5 to -3.1 % against 5 (a tile's
// fixed chain of dependent loads paid 17 % less often; 77 VGPRs, 26.4 KB LDS
// per block, still 6 blocks per CU), 7 slots (with 3 residue chunks per lane)
// no better than 5 (89 VGPRs: 5 blocks per CU), 4 slots +3.6 %
// (profiles/r05/large_tile/).
constexpr int kLaneChunksLarge = 6, kLaneChunksSmall = 3;
// Output bytes of a tile cut for `lane_chunks` slots per lane (3 slots of halo):
// 6096 for the large tile (<= 2032 residues, <= 127 residue chunks: within
// kPepSlots), 3024 for the small one.  Size any per-tile storage with the
// template's LC.
constexpr int tile_bytes(int lane_chunks) { return (64 * lane_chunks - 3) * 16; }
// plans whose large-tile count is below this use the small tile
constexpr uint64_t kSmallTilePlan = 40000;
// extraction tiles end on this output boundary where they can (bytes)
constexpr uint64_t kTileAlign = 128;
constexpr int kPepPerLane = 2;                // residue chunk slots per lane
constexpr int kHalo = 3 * kChunk;             // look-ahead decoded past the tile: codons of
                                              // the residues rounded up to a 16-byte store
constexpr int kExonCap = 128;  // intervals staged in LDS per tile (7 blocks of 4 waves fit a CU's LDS)
static_assert((kExonCap & (kExonCap - 1)) == 0, "kExonCap must be a power of two (row index masks)");
constexpr int kTxCap = 64;                    // records staged in LDS per tile
constexpr int kPepSlots = 64 * kPepPerLane;  // residue chunks per tile
constexpr uint64_t kExcBit = 1ull << 62;      // interval touches an exception run
constexpr uint64_t kSlowLitBit = 1ull << 61;  // ... whose byte has no literal class (below)
constexpr uint64_t kExFlagBits = kRcBit | kExcBit | kSlowLitBit;

// Exception bases carry a literal class in their nibble's low three bits
// (nibble = 8 | class): the bytes the kernels can write without the run
// list.  Forward strand: N n - R Y K M; any other byte is class 7 and its
// intervals take the run-list path.  The reverse-strand mirror holds the
// class of the reverse-complement literal (genome.py:787,792: N, n, - kept,
// everything else becomes n), which is always 0, 1 or 2.
__host__ __device__ constexpr uint32_t lit_class(uint32_t b) {
  return b == 'N' ? 0u : b == 'n' ? 1u : b == '-' ? 2u : b == 'R' ? 3u : b == 'Y' ? 4u
       : b == 'K' ? 5u : b == 'M' ? 6u : 7u;
}
constexpr uint32_t kLitLo = 0x522D6E4Eu;  // classes 0..3: N n - R (little-endian bytes)
constexpr uint32_t kLitHi = 0x4E4D4B59u;  // classes 4..7: Y K M (7: never written from here)

// One 16-byte output store with the non-temporal hint (global_store_dwordx4
// ... nt): the outputs are written once and never re-read by the kernel, so
// they stream through L2 instead of displacing genome lines.  A/B on one box
// (200 back-to-back C3 steps): 0.2905 -> 0.2779 ms per step (the plain-store
// variant: scripts/experiments/plain_store.patch).
__device__ __forceinline__ void store16(uint8_t* dst, uint4 v) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 x = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(x, reinterpret_cast<u32x4*>(dst));
}

// Debug switches carried in ExtractArgs.outputs (env MAGOT_DEBUG_PATHS):
// force the general per-segment / per-residue paths.
constexpr uint32_t kDebugSlowNuc = 1u << 8;
constexpr uint32_t kDebugSlowPep = 1u << 9;

// One extraction tile (a wave's work): nucleotide output bytes [T0, T1),
// residues [Q0, Q1), staged intervals [e1, e2) and records [j1, j2).  Tiles
// are stored in launch order, which is not output order: tiles that may take
// the run-list path go first (launch_order, tileplan.cpp), so their extra dependent
// loads overlap the rest of the launch instead of extending its tail.
// Host only: the device reads a tile from its TileBlock.
struct TileRec {
  uint64_t T0, T1, Q0, Q1;
  uint32_t e1, e2, j1, j2;
};
static_assert(sizeof(TileRec) == 48, "TileRec is 48 bytes");

// ---------------------------------------------------------------------------
// Packed tile descriptor blocks (tileblocks.cpp)
// ---------------------------------------------------------------------------
// Everything a wave stages for tile t, packed once per plan into block t of a
// fixed-stride table (launch order), so every load of the tile's descriptor
// has an address that follows from t alone: the header (scalar) and each
// lane's rows are one round of loads.  An interval or record staged by two
// tiles is in both blocks.  A block is
//   TileHead   T0, Q0, span | residues << 16, m | nt << 8, overflow offsets
//   ex[j]      interval e1 + j, j < min(m, ex_rows), 8 bytes (below)
//   tx[r]      record j1 + r, r <= nt, r < tx_rows: {tn - T0, tp - Q0}; row nt
//              is the sentinel (the record after the last), whose tp the
//              kernel reads.  64-bit: a record can be longer than 2^31 bases.
// The inline capacities ex_rows / tx_rows are the plan's (TileGeometry,
// tile_geometry): what nearly all of its tiles stage, so a plan of short
// tiles does not fetch blocks sized for the largest.  Rows past them (a tile
// stages up to kExonCap intervals and kTxCap + 1 record rows) are in the
// plan's overflow arrays at ovf_ex / ovf_tx: one more wave-uniform round, for
// those tiles only, one overflow row of each kind per lane (ex_rows + 64 >=
// the plan's largest m).  Rows the tile does not use are zero.
// Interval row (tile-relative, 32-bit): lo = U mod 2^32 (tile byte p reads
// unified base U + p); hi = bit 0: U bit 32, bits 1..13: end of the interval
// relative to T0, clamped to tile_bytes + 4 * kHalo, bits 14..16: reverse
// strand / exception / slow literal (kFlagRc, kFlagExc, kFlagSlowLit), bits
// 17..25: first chunk starting in the interval, ceil((o0 - T0) / 16)
// (kBlkNoChunk for row 0, which starts no chunk run).
constexpr uint32_t kFlagRc = 1u;
constexpr uint32_t kFlagExc = 2u;      // touches an exception run
constexpr uint32_t kFlagSlowLit = 4u;  // ... one without a literal class (run-list path)
constexpr uint32_t kBlkExMax = 64;  // most inline interval rows (one per lane)
constexpr uint32_t kBlkTxMax = 14;  // most inline record rows (the sentinel row included)
constexpr uint32_t kBlkNoChunk = 511;
struct TxRow {
  int64_t tn, tp;
};
struct TileHead {
  uint64_t T0, Q0;
  uint32_t span_res;  // T1 - T0 | (Q1 - Q0) << 16
  uint32_t counts;    // m | nt << 8
  uint32_t ovf_ex;    // first overflow interval row (m > ex_rows)
  uint32_t ovf_tx;    // first overflow record row (nt + 1 > tx_rows)
};
static_assert(sizeof(TileHead) == 32, "TileHead is 32 bytes");
struct TileGeometry {
  uint32_t ex_rows, tx_rows;  // inline rows: 1..kBlkExMax, 1..kBlkTxMax
  uint32_t stride;            // block bytes: header + rows, a multiple of 16
};
constexpr uint32_t tile_block_stride(uint32_t ex_rows, uint32_t tx_rows) {
  return ((uint32_t)sizeof(TileHead) + 8u * ex_rows + 16u * tx_rows + 15u) & ~15u;
}
static_assert(tile_block_stride(kBlkExMax, kBlkTxMax) == 768, "the largest block is six lines");
static_assert(kExonCap <= (int)kBlkExMax + 64 && kTxCap + 1 <= 1 + 64,
              "one inline and one overflow row per lane");
static_assert(tile_bytes(kLaneChunksLarge) + 4 * kHalo < (1 << 13) &&
              (tile_bytes(kLaneChunksLarge) + kHalo + kChunk - 1) / kChunk < (int)kBlkNoChunk,
              "interval row fields");
// The u64 tables a plan is packed from (plan_build): interval starts
// with flag bits, n+1 output offsets, record output / residue starts (n+1).
struct TileTables {
  const uint64_t* ex_g;
  const uint64_t* ex_out;
  const uint64_t* tx_nuc;
  const uint64_t* tx_pep;
  uint64_t span;
  uint32_t lane_chunks;
};
inline uint32_t tile_ovf_ex(const TileGeometry& g, const TileRec& r) {
  return r.e2 - r.e1 > g.ex_rows ? r.e2 - r.e1 - g.ex_rows : 0u;
}
inline uint32_t tile_ovf_tx(const TileGeometry& g, const TileRec& r) {
  const uint32_t rows = r.j2 > r.j1 ? r.j2 - r.j1 + 1 : 0u;
  return rows > g.tx_rows ? rows - g.tx_rows : 0u;
}
// The plan's block geometry: inline capacities that hold every row of all but
// about 2 % of the tiles (and leave at most 64 rows of either kind to the
// overflow).  force_ex / force_tx > 0 (MAGOT_TILE_BLOCK_ROWS=ex,tx: tests,
// A/Bs) replace the percentile, within the same limits.
TileGeometry tile_geometry(const TileRec* tiles, uint64_t n_tiles, uint32_t force_ex,
                           uint32_t force_tx);
// Block of tile r at b (g.stride bytes, every one written), its overflow rows
// to ovf_ex[oe ..) / ovf_tx[ot ..).
void pack_tile_block(const TileTables& tb, const TileGeometry& g, const TileRec& r, uint32_t oe,
                     uint32_t ot, uint8_t* b, uint64_t* ovf_ex, TxRow* ovf_tx);

// ---------------------------------------------------------------------------
// The extraction planner (tileplan.cpp, host only)
// ---------------------------------------------------------------------------
// From the caller's interval and record tables to the tiles, their launch
// order and the blocks' geometry: everything magot_plan_create needs before
// it allocates and uploads.  Two stages, so that the output buffers, whose
// size stage 1 gives, can be allocated while stage 2 runs.
// What the planner reads of a packed genome.
struct GenomeView {
  const uint64_t* contig_base;
  const uint64_t* contig_len;
  uint64_t n_contigs;
  uint64_t span;
  const ExcRun* runs;   // host run list, sentinel appended
  const uint32_t* dir;  // its block directory
};
struct PlanOptions {
  uint32_t outputs;      // MAGOT_OUT_NUC | MAGOT_OUT_PEP
  bool by_genome;        // MAGOT_OUT_GENOME_ORDER
  int lane_chunks;       // MAGOT_EXTRACT_LANE_CHUNKS (0: the planner's choice)
  uint32_t block_ex, block_tx;  // MAGOT_TILE_BLOCK_ROWS=ex,tx (0: the planner's choice)
};
// The tables are there and fit one plan, the output flags are known.
int plan_check_tables(const magot_exon* exons, uint64_t n_exons, const magot_tx* txs,
                      uint64_t n_tx, uint32_t outputs);
// `outputs` as given to magot_plan_create, and the environment's overrides.
PlanOptions plan_options(uint32_t outputs);
struct PlanInput {
  GenomeView g;
  const magot_exon* exons;
  uint64_t E;
  const magot_tx* txs;
  uint64_t T;
  PlanOptions opt;
};
// Stage 1: record t's compacted (non-empty) intervals are [rec_ex[t],
// rec_ex[t+1]) of Ec, its length rec_len[t]; B output bytes, P residues.
struct PlanCount {
  std::vector<uint64_t> rec_ex, rec_len;
  uint64_t Ec = 0, B = 0, P = 0;
  unsigned nth = 1;  // host threads over record ranges (large plans)
};
int plan_count(const PlanInput& in, PlanCount* out);
// Stage 2: the u64 tables in layout order (TileTables), each record's place,
// the tiles in launch order and where their blocks' overflow rows go.
struct TilePlan {
  HostBuf<uint64_t> ex_g, ex_out;    // Ec + 1 starts with flag bits, Ec + 2 output offsets
  std::vector<uint64_t> tn, tp;      // records with a codon, Tc + 1 (sentinel B, P)
  std::vector<uint64_t> nuc_off, pep_off;  // record-order prefix offsets, T + 1
  std::vector<uint64_t> lay_nuc, lay_pep;  // each record's place in the layout, T
  uint64_t Ec = 0, Tc = 0;
  uint32_t lane_chunks = 0;
  std::vector<TileRec> tiles;        // launch order
  TileGeometry geo{};
  std::vector<uint32_t> ovf_at;      // tile t's first overflow interval / record row
  uint64_t n_ovf_ex = 0, n_ovf_tx = 0;
  unsigned nth = 1;
};
int plan_build(const PlanInput& in, PlanCount&& cnt, Lap& lap, TilePlan* out);
// The cut: the output [0, ex_out[Ec]) as tiles of at most `tile` bytes
// (tile_bytes), appended to *tiles in output order.
int cut_tiles(const uint64_t* ex_out, uint64_t Ec, const uint64_t* tn, const uint64_t* tp,
              uint64_t Tc, uint64_t tile, std::vector<TileRec>* tiles);

// Device plan.  Zero-length intervals and records without a codon are
// compacted away on the host (they add no output); tiles are 16-byte aligned
// ranges of the nucleotide output of at most tile_bytes(lane_chunks) bytes, cut shorter where
// they would touch more than kExonCap intervals or kTxCap records.
struct ExtractArgs {
  // Nibble plane in unified coordinates: [0, span) forward strand, [span,
  // 2*span) reverse strand, where u = 2*span-1-g holds the complement of g.
  const uint32_t* nib;
  uint64_t span;
  const ExcRun* runs;
  const uint32_t* dir;
  const uint8_t* blocks;      // n_tiles blocks of blk.stride bytes, in launch order
  const uint64_t* ovf_ex;     // interval rows past a block's blk.ex_rows
  const TxRow* ovf_tx;        // record rows past a block's blk.tx_rows
  TileGeometry blk;
  uint8_t* nuc;
  uint8_t* pep;
  uint64_t total_nuc;
  uint64_t total_pep;
  uint32_t n_tiles;
  uint32_t outputs;
  uint32_t lut[16];           // 64 residue bytes indexed c0 + 4*c1 + 16*c2
  uint32_t lane_chunks;       // tile size the plan was cut for (kLaneChunksLarge / Small)
};

// Wave-wide inclusive prefix sum with DPP row shifts and row broadcasts
// (gfx9 wave64: row_shr:1/2/4/8 inside rows of 16, then row_bcast:15/31).
// The row_bcast controls exist only on gfx9 (CDNA) wave64 targets.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#error "wave_scan uses DPP row_bcast:15/31, which exists only on gfx9 wave64 (gfx950) targets"
#endif
__device__ __forceinline__ uint32_t wave_scan(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);
  return v;
}

// bit k: byte k of x equals the byte repeated in pat (SWAR: no carry leaves a byte)
__device__ __forceinline__ uint32_t byte_eq_mask4(uint32_t x, uint32_t pat) {
  x ^= pat;
  const uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
  const uint32_t z = ~(t | x | 0x7f7f7f7fu) >> 7;
  return (z * 0x00204081u) >> 21 & 0xFu;
}

// bit k: byte k of the 16 bytes of v equals the byte repeated in pat
__device__ __forceinline__ uint32_t byte_eq_mask16(uint4 v, uint32_t pat) {
  return byte_eq_mask4(v.x, pat) | byte_eq_mask4(v.y, pat) << 4 | byte_eq_mask4(v.z, pat) << 8 |
         byte_eq_mask4(v.w, pat) << 12;
}

// Dynamic LDS (never touched by the kernel) that caps a kernel at `want`
// resident blocks per CU; 0 when it already fits or want <= 0.
inline size_t occupancy_lds_pad(const void* fn, int threads, int want) {
  if (want <= 0) return 0;
  int dev = 0, lds_cu = 0, n = 0;
  hipFuncAttributes at{};
  if (hipGetDevice(&dev) != hipSuccess || hipFuncGetAttributes(&at, fn) != hipSuccess ||
      hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) !=
          hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, threads, 0) != hipSuccess || n <= want)
    return 0;
  const size_t need = (size_t)lds_cu / (size_t)(want + 1) + 1;  // > 1/(want+1) of the CU's LDS
  return need > at.sharedSizeBytes ? need - at.sharedSizeBytes : 0;
}

void launch_extract(const ExtractArgs& a, hipStream_t s);
int extract_blocks_per_cu();
// Fill the reverse-strand half of the nibble plane.
void launch_mirror_planes(uint32_t* nib, uint64_t span, hipStream_t s);

// ---------------------------------------------------------------------------
// Raw sequence batch ops (seqops.hip)
// ---------------------------------------------------------------------------
void launch_revcomp(const uint8_t* in, const uint64_t* off, uint64_t n, uint64_t total,
                    uint8_t* out, hipStream_t s);
// Six translations per record for Sequence.get_orfs (orf6_kernel): stream
// j = 6*record + 2*frame + (strand == '+'); boff = n_rec+1 offsets of each
// record's block of six 16-byte padded streams (strand-major inside the block,
// magot_orf6_sizes; the kernel derives each stream's place from the record's
// length); noff = n_rec+1 offsets of the records in the concatenation.
// The records are either bytes (nuc, readable up to the next 16-byte
// boundary) or gathered from the genome plane through interval rows
// {unified anchor, start} (n_rows + a sentinel row {0, total}): base P of
// the concatenation is unified coordinate anchor + P of its interval.
// Tiles (orf6_plan_tiles): t0 = n_tiles+1 starts, r0 = record holding each
// start, e0 = interval holding each staged window's first base.
constexpr uint32_t kOrf6RowCap = 123;  // intervals per staged window
constexpr uint64_t kOrf6ExcRow = 1ull << 63;  // row start flag: the interval touches an exception run
struct Orf6Args {
  const uint8_t* nuc;
  const uint32_t* nib;
  uint64_t nib_words;      // both planes
  const uint32_t* code2;   // 2-bit codes of the same unified bases, 16 per word
  uint64_t code2_words;    // = nib_words / 2
  const uint32_t* exc1;    // exception bits of the same unified bases, 32 per word
  uint64_t exc1_words;     // = nib_words / 4
  const uint64_t* rows;
  uint64_t n_rows;
  const uint64_t* noff;
  uint64_t n_rec;
  uint64_t total;
  const uint64_t* boff;
  const uint64_t* tile_t0;
  const uint32_t* tile_r0;
  const uint32_t* tile_e0;
  const uint32_t* tile_m;  // rows of the tile's window (interval starts before its end), <= kOrf6RowCap
  uint64_t n_tiles;
  const uint8_t* tables;  // 256 bytes from orf6_tables
  uint8_t* out;
};
struct Orf6Tiles {
  std::vector<uint64_t> t0;
  std::vector<uint32_t> r0, e0, m;
};
void orf6_tables(const uint8_t lut64[64], uint8_t out[256]);
void orf6_plan_tiles(const uint64_t* noff, uint64_t n_rec, const uint64_t* row_start,
                     uint64_t n_rows, Orf6Tiles* out);
void launch_orf6(const Orf6Args& a, bool genome, hipStream_t s);
// The 2-bit code plane of a nibble plane (nib_words words, 8 bases each):
// word w holds the codes of unified bases 16w .. 16w+15 (base k at bits 2k).
void launch_code2(const uint32_t* nib, uint64_t nib_words, uint32_t* code2, hipStream_t s);
// The exception-bit plane: word w holds bit 3 of the nibbles of unified bases
// 32w .. 32w+31 (base k at bit k).
void launch_exc1(const uint32_t* nib, uint64_t nib_words, uint32_t* exc1, hipStream_t s);
void launch_translate(const uint8_t* in, const uint64_t* off, uint64_t n, const int32_t* frames,
                      const uint8_t* strands, const uint64_t* pep_off, uint64_t total_pep,
                      const uint32_t* lut16, uint8_t* out, hipStream_t s);
// Codon symbols over an extended alphabet (magot_codon_symbols): K classes,
// K^3 <= kMaxSymbolLut.
constexpr uint32_t kMaxSymbolLut = 32768;
void launch_codon_symbols(const uint8_t* in, uint64_t n_codons, const uint8_t* cls, uint32_t K,
                          const uint8_t* lut, uint8_t* out, hipStream_t s);

// ---------------------------------------------------------------------------
// FASTA text assembly (render.hip, gffplan.cpp)
// ---------------------------------------------------------------------------
// A run of skeleton text followed by at most one record payload.
constexpr uint32_t kNoRecord = 0xFFFFFFFFu;
struct TextUnit {
  uint64_t text_off;
  uint32_t text_len;
  uint32_t rec;  // record index, or kNoRecord
};
// Record indices in ascending key order, ties in index order (pack.cpp;
// magot_plan_create's genome-order layout).  key.size() < 2^32.
void radix_order(const std::vector<uint64_t>& key, std::vector<uint32_t>* out);
// The planner's skeleton as units (consecutive text pieces merged).
// Returns false when a record index does not fit a TextUnit.
bool gffplan_units(const magot_gffplan* p, const std::string** text, std::vector<TextUnit>* units,
                   bool* protein, uint64_t* n_rec);
size_t text_scan_bytes(uint64_t n);
void launch_text_assembly(const TextUnit* units, uint64_t n, const uint64_t* rspan,
                          const uint8_t* pay, int protein, const uint8_t* text, uint64_t* len,
                          uint64_t* psrc, uint64_t* end, void* scan_tmp, size_t scan_bytes,
                          uint8_t* out, hipStream_t s);

// ---------------------------------------------------------------------------
// ORF calling over the six-frame streams (orfcall.hip; magot_orfcall_*)
// ---------------------------------------------------------------------------
constexpr uint32_t kOrfCallTile = 1024;  // residues per tile: 16 per lane of one wave
constexpr uint8_t kOrfFlagNone = 1;       // a stream whose translate() is None
constexpr uint8_t kOrfFlagNoLongest = 2;  // longest: every output string is empty
constexpr uint32_t kOrfDigits = 12;       // scratch bytes per ORF: decimal position + '\n'
struct OrfCallArgs {
  uint32_t mode;             // MAGOT_ORF_*
  const uint8_t* res;        // the six-frame kernel's output
  const uint64_t* soff;      // 6n + 1 stream offsets, record order, loop order inside
  const uint64_t* noff;      // n + 1 record offsets (for the record lengths)
  uint64_t n_rec;
  uint32_t* scnt;            // 6n + 1: tiles per stream (the last entry 0)
  uint64_t* tile_first;      // 6n + 1: their prefix
  uint8_t* flags;            // n: kOrfFlag*
  uint64_t n_tiles;
  uint32_t* tile_stream;     // n_tiles: 6 * record + j
  uint32_t *orfs, *kept;     // n_tiles + 1: ORFs owned, output bytes
  uint32_t* extra;           // from_atg: more bytes when the running ORF has had its M
  uint8_t *tflags, *tseen;   // from_atg: the tile's marks; the carried bit
  uint64_t *obase, *kbase;   // n_tiles + 1: prefixes of orfs / kept
  uint64_t n_orfs;
  uint32_t* rec;             // the table, n_orfs rows
  uint8_t* j;
  uint32_t *k, *len;
  uint64_t* poff;
  uint8_t* payload;
  // longest
  uint64_t* sel;             // n: the chosen ORF
  uint32_t *valid, *sellen;  // n + 1
  uint64_t *slot, *cpoff;    // n + 1: prefixes of valid / sellen
  uint64_t n_sel;
  uint32_t* c_rec;           // the chosen rows, n_sel
  uint8_t* c_j;
  uint32_t *c_k, *c_len;
  uint64_t* c_poff;
  uint8_t* c_payload;
  uint64_t *src_off, *dst_off;  // n_sel, n_sel + 1: the payload's segment copy
  void* scan_tmp;
  size_t scan_bytes;
};
struct OrfTextArgs {
  int longest;
  uint64_t n;                // entries (ORFs, or chosen rows)
  const uint32_t* rec;
  const uint8_t* j;
  const uint32_t *k, *len;
  const uint64_t* poff;
  const uint8_t* payload;
  const uint64_t* noff;
  const uint64_t* hoff;      // n_rec + 1: each record's '\n' + header in text
  uint8_t* text;             // the headers, then kOrfDigits bytes per entry at dig_off
  uint64_t dig_off;
  uint32_t* tlen;            // n + 1
  uint64_t* tstart;          // n + 1
  uint8_t* out;
  void* scan_tmp;
  size_t scan_bytes;
};
size_t orfcall_scan_bytes(uint64_t n);
hipError_t launch_orfcall_streams(const OrfCallArgs& a, hipStream_t s);
hipError_t launch_orfcall_count(const OrfCallArgs& a, hipStream_t s);
hipError_t launch_orfcall_write(const OrfCallArgs& a, hipStream_t s);
hipError_t launch_orfcall_longest(const OrfCallArgs& a, hipStream_t s);
hipError_t launch_orfcall_compact(const OrfCallArgs& a, hipStream_t s);
hipError_t launch_orftext_sizes(const OrfTextArgs& a, hipStream_t s);
hipError_t launch_orftext_copy(const OrfTextArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------
// The longest ORF of every record of a plan's nucleotide output, fused
// (longorf.hip; magot_longorf_*)
// ---------------------------------------------------------------------------
constexpr uint32_t kLongOrfStep = 64;  // codons per step: one per lane of a wave
struct LongOrfArgs {
  const uint8_t* nuc;     // the plan's nucleotide output
  const uint64_t* start;  // n: each record's first byte in nuc (the plan's layout)
  const uint64_t* noff;   // n + 1 record offsets (for the record lengths, all < 2^32)
  uint64_t n;
  const uint8_t* lut;     // 64: the library, c0 + 4*c1 + 16*c2 with A=0 C=1 G=2 T=3
  uint32_t waves;         // launched, a multiple of 4; each strides over the records
  uint8_t* j;             // n: the winner's stream
  uint32_t* k;            // n: its start residue (behind a trimmed leading 'X')
  uint32_t* ku;           // n: its first codon in the stream (the trimmed one counted)
  uint32_t* len;          // n + 1: its residues, 0 for a flagged record; the last entry 0
  uint8_t* flags;         // n: 0 or kOrfFlagNoLongest
  uint64_t* poff;         // n + 1: prefix of len
  uint8_t* payload;       // poff[n] bytes
  void* scan_tmp;
  size_t scan_bytes;
};
struct LongOrfTextArgs {
  uint64_t n_print;          // entries: records [0, n_print)
  const uint64_t* name_off;  // n_print + 1
  const uint8_t* names;
  uint32_t* tlen;            // n_print + 1: bytes of each entry, the last entry 0
  uint64_t* tstart;          // n_print + 1: their prefix
  uint8_t* out;
  void* scan_tmp;
  size_t scan_bytes;
};
size_t longorf_scan_bytes(uint64_t n);
hipError_t launch_longorf_call(const LongOrfArgs& a, hipStream_t s);   // winners, then poff
hipError_t launch_longorf_write(const LongOrfArgs& a, hipStream_t s);  // the payload
hipError_t launch_longorf_text_sizes(const LongOrfArgs& a, const LongOrfTextArgs& t, hipStream_t s);
hipError_t launch_longorf_text_write(const LongOrfArgs& a, const LongOrfTextArgs& t, hipStream_t s);

// ---------------------------------------------------------------------------
// mask_from_gff (maskplan.cpp, maskgen.hip; magot_mask_*)
// ---------------------------------------------------------------------------
constexpr uint32_t kMaskPiece = 2048;  // most bases of one interval piece (maskplan.cpp)
struct MaskArgs {
  uint32_t flags;                  // MAGOT_MASK_*
  const uint8_t* src;              // the whole-contig extraction's nucleotide output
  uint64_t src_bytes;              // its size = bits of the coverage plane
  const magot_mask_interval* rows; // n_rows interval pieces
  uint64_t n_rows;
  const uint64_t* contig_src;      // per contig: its first byte in src
  uint32_t* cov;                   // cov_words + 1 words (the text pass reads word pairs)
  uint64_t cov_words;
  uint64_t n_rec;                  // contigs in output order
  const uint64_t* tstart;          // n_rec + 1: each record's first text byte, and the total
  const uint64_t* rsrc;            // n_rec: each record's first byte in src
  const uint32_t* hlen;            // n_rec: header bytes ('>' name '\n')
  const uint64_t* hoff;            // n_rec: the header's place in hdr
  const uint8_t* hdr;
  uint8_t* out;
  uint64_t text_bytes;
};
hipError_t launch_mask_paint(const MaskArgs& a, hipStream_t s);
hipError_t launch_mask_text(const MaskArgs& a, hipStream_t s);
// The paint kernel alone, into a plane of n_bits bits that is not zeroed first:
// the pieces' bits are OR-ed into what it holds (track.hip's paint).
hipError_t launch_mask_paint_rows(const magot_mask_interval* rows, uint64_t n_rows,
                                  const uint64_t* contig_src, uint32_t* cov, uint64_t n_bits,
                                  hipStream_t s);

// ---------------------------------------------------------------------------
// position_dic's bit track (track.hip; magot_track_*)
// ---------------------------------------------------------------------------
// One bit per base over the genome's forward coordinates [0, span): bit g & 31
// of word g >> 5; every bit outside [kOrigin, extent) is zero.  The plane is
// allocated in whole rank blocks (track_plane_words).
// Rank directory: ones per block of kRankWords words and their exclusive
// prefix.  16 words = 512 bases = 64 bytes: a rank reads one directory entry
// and at most four 16-byte loads that never leave one 64-byte half line, and
// the directory (4 bytes per block) adds 1/16 to the plane.
constexpr int kRankWords = 16;
constexpr uint64_t track_blocks(uint64_t span) { return (span / 32 + kRankWords - 1) / kRankWords; }
constexpr uint64_t track_plane_words(uint64_t span) { return (track_blocks(span) + 1) * kRankWords; }
struct TrackWindowArgs {
  const uint32_t* track;
  const uint32_t* rank;         // track_blocks + 1 entries
  const uint64_t* contig_base;  // n_contigs
  const uint64_t* first;        // n_contigs + 1: each contig's first window, and the total
  uint64_t n_contigs;
  uint64_t n_windows;
  uint64_t W, jump;
  uint32_t* sums;               // n_windows
  uint32_t* flip_count;         // track_flip_groups(n_windows) + 1
  uint64_t* flip_slot;          // the same number: exclusive prefix, the last entry the total
  uint64_t* flip_index;         // the windows where the threshold test flips
};
constexpr uint64_t track_flip_groups(uint64_t n_windows) { return (n_windows + 63) / 64; }
size_t track_scan_bytes(uint64_t n);
// the A/T (gc false) or C/G class of the forward nibble plane, n_words = span / 32
// words, the bases outside [lo, hi) cleared; OR-ed into `track` or replacing it
hipError_t launch_track_class(const uint32_t* nib, uint64_t n_words, uint64_t lo, uint64_t hi,
                              bool gc, bool replace, uint32_t* track, hipStream_t s);
hipError_t launch_track_andnot(uint32_t* track, const uint32_t* clear, uint64_t n_words,
                               hipStream_t s);
// coordinates [lo, hi) from / to a byte per base staged at stage[(lo & 31) + i]
// (32 * words touched bytes, 16-byte aligned)
hipError_t launch_track_bytes_set(const uint8_t* stage, uint64_t lo, uint64_t hi, uint32_t* track,
                                  hipStream_t s);
hipError_t launch_track_bytes_get(const uint32_t* track, uint64_t lo, uint64_t hi, uint8_t* stage,
                                  hipStream_t s);
hipError_t launch_track_rank(const uint32_t* track, uint64_t n_blocks, uint32_t* count,
                             uint32_t* rank, void* scan_tmp, size_t scan_bytes, hipStream_t s);
hipError_t launch_track_windows(const TrackWindowArgs& a, hipStream_t s);
hipError_t launch_track_flip_count(const TrackWindowArgs& a, uint32_t s_min, void* scan_tmp,
                                   size_t scan_bytes, hipStream_t s);
hipError_t launch_track_flip_write(const TrackWindowArgs& a, uint32_t s_min, uint64_t cap,
                                   hipStream_t s);
hipError_t launch_track_count(const magot_mask_interval* rows, uint64_t n_rows,
                              const uint64_t* contig_base, const uint32_t* track,
                              const uint32_t* rank, uint64_t span, uint32_t* ones, hipStream_t s);

// ---------------------------------------------------------------------------
// depth_from_gff's integer track (depth.hip; magot_depth_*)
// ---------------------------------------------------------------------------
// The depth column of a `samtools depth` table as one int32 per line, in line
// order (the arena, allocated in whole directory blocks plus one), and the
// directory: int64 sums per kDepthBlock depths and their exclusive prefix.
// 256 depths = 1 KiB: a prefix reads one directory entry and at most 64
// 16-byte loads of one block; the directory adds 1/128 to the arena.
constexpr int kDepthBlock = 256;
constexpr uint64_t depth_blocks(uint64_t n_lines) { return (n_lines + kDepthBlock - 1) / kDepthBlock; }
// what links a chunk to the next: the lines so far, and the last line's name
// and position
struct DepthCarry {
  uint64_t lines;
  uint32_t has_prev, name_len, pos, pad;
  uint8_t name[256];
};
struct DepthHead {  // a run's first line
  uint64_t line, offset;  // offset: of the name in the file
  uint32_t name_len, pad;
};
struct DepthParseArgs {
  const uint8_t* text;  // the chunk, 16-byte aligned, starting at a line start
  int64_t n;            // its bytes (> 0)
  uint64_t file_off;    // its place in the file
  const uint32_t* blk_first;  // depth_text_blocks(n) + 1: LFs before each text block, the total
  const DepthCarry* in;
  DepthCarry* out;      // not `in`
  int32_t* arena;
  uint64_t arena_cap;   // lines the arena holds
  DepthHead* heads;
  uint32_t* n_heads;    // counts every run head, stored or not
  uint32_t heads_cap;
  unsigned long long* status;  // min of (line << 8 | MAGOT_DEPTH_* reason); ~0 when clean
};
size_t depth_scan_bytes(uint64_t n);
hipError_t launch_depth_line_index(const uint8_t* text, uint64_t n, uint32_t* count,
                                   uint32_t* first, void* scan_tmp, size_t scan_bytes,
                                   hipStream_t s);
hipError_t launch_depth_parse(const DepthParseArgs& a, hipStream_t s);
hipError_t launch_depth_directory(const int32_t* arena, uint64_t n_lines, int64_t* block_sum,
                                  int64_t* dir, void* scan_tmp, size_t scan_bytes, hipStream_t s);
hipError_t launch_depth_sums(const int32_t* arena, const int64_t* dir, uint64_t n_lines,
                             const int64_t* start, const int64_t* length, uint64_t n_rows,
                             int64_t* sums, hipStream_t s);
hipError_t launch_depth_groups(const int64_t* sums, const uint64_t* offsets, uint64_t n_groups,
                               int64_t* out, hipStream_t s);

// ---------------------------------------------------------------------------
// fqstats' read-length histogram (fastq.hip; magot_fq_*)
// ---------------------------------------------------------------------------
// Lengths below kFqDense are counted in uint64 hist[kFqDense]; a longer one is
// appended to a list (such a line has at least kFqDense bytes of text, so the
// list is bounded by the file's size).
constexpr uint64_t kFqDense = 1ull << 20;
constexpr uint64_t fq_long_cap(uint64_t file_bytes) { return file_bytes / kFqDense + 2; }
// per text block, and after the scan the blocks before it: LFs, and the file
// offset of the last LF (-1: none)
struct FqBlock {
  uint64_t lines;
  int64_t last_lf;
};
typedef FqBlock FqCarry;  // the same over the chunks before: what links a chunk to the next
struct FqItem {  // running totals of the descending walk
  uint64_t count, bases;
};
struct FqChunkArgs {
  const uint8_t* text;  // the chunk, 16-byte aligned; cut anywhere
  int64_t n;            // its bytes (> 0)
  int64_t file_off;     // its place in the file
  FqBlock* blk;         // depth_text_blocks(n) + 1: the blocks' own values, the last one empty
  FqBlock* pre;         // their exclusive scan; entry depth_text_blocks(n) is the chunk's total
  const FqCarry* in;
  FqCarry* out;         // not `in`
  unsigned long long* hist;       // kFqDense bins
  int64_t* longs;                 // lengths >= kFqDense
  unsigned long long* n_longs;    // counts every one, stored or not
  uint64_t longs_cap;
};
struct FqReduceArgs {
  const unsigned long long* hist;
  const int64_t* longs;  // descending
  uint64_t n_longs;
  FqItem* cum;           // n_longs + kFqDense
  uint64_t* out;         // 9: reads, bases, median, 25 % and 75 % marks, n25, n50, n75, and
                         // which of the last three were set (bits 0..2); zero before the launch
};
size_t fq_scan_bytes(uint64_t n_blocks, uint64_t n_items);
size_t fq_sort_bytes(uint64_t n);
unsigned fq_grid(uint64_t n, int n_cu);
hipError_t launch_fq_line_index(const FqChunkArgs& a, void* scan_tmp, size_t scan_bytes,
                                hipStream_t s);
hipError_t launch_fq_lengths(const FqChunkArgs& a, unsigned grid, hipStream_t s);
hipError_t launch_fq_tail(const FqChunkArgs& a, uint64_t file_bytes, hipStream_t s);
hipError_t launch_fq_sort(const int64_t* in, int64_t* out, uint64_t n, void* tmp, size_t bytes,
                          hipStream_t s);
hipError_t launch_fq_reduce(const FqReduceArgs& a, void* scan_tmp, size_t scan_bytes,
                            hipStream_t s);

// ---------------------------------------------------------------------------
// Interval joins: purge_overlaps, annotation_overlap (overlap.hip;
// magot_overlap_*)
// ---------------------------------------------------------------------------
// Composite key of one interval end: dense seqid above the coordinate biased
// to unsigned, so one sorted table holds every seqid's ends as one segment
// each.  The all-ones key (seqid 2^24 - 1) marks an interval left out of a
// table and sorts behind every segment.
constexpr int kOvCoordBits = 40;
constexpr int64_t kOvCoordMin = -(1ll << (kOvCoordBits - 1));
constexpr int64_t kOvCoordMax = (1ll << (kOvCoordBits - 1)) - 1;
constexpr uint32_t kOvMaxSeq = (1u << (64 - kOvCoordBits)) - 1;  // seqids 0 .. kOvMaxSeq - 1
constexpr uint32_t kOvNoSeq = 0xffffffffu;  // a query on a seqid the index does not hold
// overlap's range scan: a query with at most kOvLaneScan intervals starting
// inside it is scanned by its own lane, a longer one by a whole wave
constexpr uint32_t kOvLaneScan = 64;
__host__ __device__ inline uint64_t ov_key(uint32_t seq, int64_t x) {
  return ((uint64_t)seq << kOvCoordBits) | (uint64_t)(x - kOvCoordMin);
}
// The three tables of an index of n intervals, each of n keys with the left
// out ones behind, and each table's segment bounds (n_seq + 1 entries):
//   in    p0 < p1   starts and ends           purge's first two tests
//   all   every     starts                    purge's third test
//   cl    p0 <= p1  starts with their ends, and ends   overlap
struct OvIndex {
  uint64_t n;
  uint32_t n_seq;
  const uint64_t *in_s, *in_e, *all_s, *cl_s, *cl_e;
  const int64_t* cl_v;  // the end of the interval whose start is cl_s[i]
  const uint64_t *seg_in, *seg_all, *seg_cl;
};
struct OvBuildArgs {
  uint64_t n;
  uint32_t n_seq;
  const uint32_t* seq;     // n, each < n_seq
  const int64_t *p0, *p1;  // n, each in [kOvCoordMin, kOvCoordMax]
  // unsorted keys (5 n) and ends (n), then the sorted tables of OvIndex
  uint64_t* raw;
  int64_t* raw_v;
  uint64_t *in_s, *in_e, *all_s, *cl_s, *cl_e;
  int64_t* cl_v;
  uint64_t *seg_in, *seg_all, *seg_cl;
};
struct OvQuery {
  uint64_t n;
  const uint32_t* seq;     // n; kOvNoSeq or >= n_seq: no partner
  const int64_t *c0, *c1;  // n, each in [kOvCoordMin, kOvCoordMax]
};
size_t ov_sort_bytes(uint64_t n);
hipError_t launch_ov_keys(const OvBuildArgs& a, hipStream_t s);
hipError_t launch_ov_sort(const OvBuildArgs& a, void* tmp, size_t bytes, hipStream_t s);
hipError_t launch_ov_segments(const OvBuildArgs& a, hipStream_t s);
hipError_t launch_ov_purge(const OvIndex& ix, const OvQuery& q, uint8_t* drop, hipStream_t s);
// counts: n; long_list: n; n_long: one counter, zeroed here
hipError_t launch_ov_overlap(const OvIndex& ix, const OvQuery& q, int64_t* counts,
                             uint32_t* long_list, unsigned long long* n_long, int n_cu,
                             hipStream_t s);

// ---------------------------------------------------------------------------
// besthits_from_psl: a reduction keyed by a string (psl.hip; magot_psl_*)
// ---------------------------------------------------------------------------
// rank of a data line: its score biased to unsigned above the line counted
// from the top, so the maximum over a key is the highest score and, among
// equals, the earliest line; a stable sort of ranks in line order keeps each
// key's lines in line order.
constexpr uint64_t kPslLineMask = (1ull << 31) - 1;  // lines 0 .. 2^31 - 2
__host__ __device__ inline uint64_t psl_rank(int64_t score, uint64_t line) {
  return ((uint64_t)(score + (1ll << 31)) << 31) | (kPslLineMask - line);
}
__host__ __device__ inline uint64_t psl_rank_line(uint64_t rank) {
  return kPslLineMask - (rank & kPslLineMask);
}
__host__ __device__ inline int64_t psl_rank_score(uint64_t rank) {
  return (int64_t)(rank >> 31) - (1ll << 31);
}
struct PslAgg {  // per key: the best rank, and the rank's low bits of its first line
  uint64_t best, first;
};
struct PslArgs {
  TextIndexArgs ix;     // the text and its line index: ix.pos[k] is where line k starts
  // per line, ix.n_lines of each
  uint64_t* hash;       // CPython 2.7's hash of the key (data lines)
  uint64_t* key_off;
  uint32_t* key_len;
  uint64_t* rank;
  uint32_t* kind;       // 1: data line, 0: pass-through; then n_lines + 1 of
  uint32_t* dpos;       // their exclusive scan: data lines before each line
  unsigned long long* status;  // min of (line << 8 | MAGOT_PSL_* reason); ~0 when clean
  // the data lines compacted (n_data), then sorted by the masked hash
  uint64_t n_data;
  uint32_t hash_bits;
  uint64_t *skey, *sval, *skey_sorted, *sval_sorted;
  uint64_t *pass_off, *pass_len;  // n_lines - n_data, in file order
  // per key (n_groups, at most n_data)
  uint64_t n_groups;
  uint64_t* uniq;       // the masked hashes that occur
  PslAgg* agg;
  unsigned long long* n_uniq;
  uint32_t *seg_first, *seg_id, *seg_first_sorted, *seg_id_sorted;
  // the rows of magot_psl_groups, in first-seen order
  uint64_t *g_hash, *g_off, *g_len;
  int64_t* g_score;
  uint32_t *g_first, *g_best;
};
// rocprim scratch of every pass over a text of n_lines lines (n_data and n_groups
// are at most n_lines)
size_t psl_tmp_bytes(uint64_t n_lines);
hipError_t launch_psl_parse(const PslArgs& a, hipStream_t s);
hipError_t launch_psl_compact(const PslArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_psl_scatter(const PslArgs& a, hipStream_t s);
hipError_t launch_psl_sort(const PslArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_psl_verify(const PslArgs& a, hipStream_t s);
hipError_t launch_psl_reduce(const PslArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_psl_order(const PslArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s);

// ---------------------------------------------------------------------------
// composition_by_site (sitecount.hip; genome_tools.py:488-503)
// ---------------------------------------------------------------------------
// Per site of an alignment whose rows lie in the forward nibble plane, the
// rows that hold a, t, c, g there (either case).  A lane owns kSiteLane
// consecutive sites, one word of every row after a funnel shift by the row's
// start; a workgroup owns a tile of sites and a strip of rows.  Per code a
// 0/1-per-nibble mask is added into 4-bit counters, which are widened into
// bytes every kSiteWiden4 rows (15 is the most a nibble holds) and the bytes
// into 32-bit registers every kSiteWiden8 rows (17 * 15 = 255, the most a byte
// holds).  One strip: the counts are stored; several: added with integer
// atomics into zeroed memory, exact in any order.
constexpr uint32_t kSiteLane = 8;
constexpr uint32_t kSiteBlock = 256;
constexpr uint32_t kSiteTile = kSiteLane * kSiteBlock;
constexpr uint32_t kSiteWiden4 = 15;
constexpr uint32_t kSiteWiden8 = 17 * kSiteWiden4;
constexpr uint32_t kSiteStrip = 4 * kSiteWiden8;
struct SiteArgs {
  const uint32_t* nib;        // the forward plane
  const uint64_t* row_start;  // n_rows global base coordinates
  uint64_t n_rows, n_sites;
  uint32_t* counts;           // n_sites x 4: a, t, c, g
  uint32_t n_tiles, n_strips;
};
// zeroes the counts first when there are several strips
hipError_t launch_site_count(const SiteArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------
// heterozygosity_from_vcf (vcf.hip; magot_variants.py:16-139; magot_vcf_*)
// ---------------------------------------------------------------------------
// The text is resident and indexed by textindex.hip's line index.  Data lines are
// compacted, parsed a wave each into (POS, key hash, CHROM run head, one het bit
// per sample column), keyed (contig << 32 | POS) once the host has named the
// runs' contigs, and sorted; a locus is a range of the sorted keys.
constexpr uint32_t kVcfMaxSamples = 1024;  // the parse kernel's LDS: column starts and the field table
constexpr uint32_t kVcfTable = 4096;       // its slots: the power of two above 2 * (9 + kVcfMaxSamples)
constexpr uint32_t kVcfSplit = 4096;       // sorted rows one workgroup of the counting pass goes down
constexpr uint32_t kVcfMaxRuns = 1u << 20; // CHROM runs the host names one by one
constexpr uint64_t kVcfMaxCounts = 1ull << 29;  // loci x samples (2 GiB of counters)
struct VcfArgs {
  const uint8_t* text;  // n bytes, 16-byte aligned, readable to the next multiple of 16 and 16 more
  uint64_t n;
  uint64_t n_lines;
  uint32_t final_lf;             // 1: the text's last byte is LF (every line has one)
  const uint64_t* line_start;  // n_lines + 1 (TextIndexArgs::pos, line mode)
  // per line: 1 for a data line, 1 << 32 for a "##" line; n_lines + 1, the last 0
  uint64_t* kind;
  uint64_t* kpos;  // their exclusive scan: both counts before each line, the totals last
  // [0] min of (line << 8 | MAGOT_VCF_* reason), ~0 when clean; [1] the '#' lines
  // that are not "##"; [2] the first of them; [3] the first data line; [4] 1 when
  // the text holds a CR
  unsigned long long* status;
  uint64_t n_data, n_hdr;
  uint32_t n_samples, words;  // words = ceil(n_samples / 32)
  uint32_t* data_line;  // n_data: the line of each data line
  uint64_t *hdr_off, *hdr_len;  // n_hdr: the "##" lines without their LFs, in file order
  // per data line
  int32_t* pos;
  uint64_t* hash;       // CPython 2.7's string hash of CHROM + "<:>" + POS
  uint32_t* chrom_len;
  uint32_t* head;       // n_data + 1: 1 where CHROM differs from the data line before; the last 0
  uint32_t* run;        // their exclusive scan; run[n_data]: the runs
  uint32_t* bits;       // n_data x words: bit s: column s is the line's first field with its
                        // bytes and its GT's first and last byte differ
  uint64_t n_runs;
  uint64_t *run_off, *run_len;  // n_runs: the CHROM span of each run's first line
  // after the host has named the runs
  const uint32_t* contig_of_run;  // n_runs
  uint32_t key_bits;
  uint64_t *key, *key_sorted;     // n_data
  uint32_t *val, *val_sorted;     // the data line of each key; sorted stably
  uint8_t* kept_sorted;           // 1: the last line of its key
  uint8_t *kept, *first;          // per data line: the last, the first line of its key
};
struct VcfCountArgs {
  uint64_t n_loci;
  const uint32_t *contig, *lo, *hi;  // n_loci; lo > hi: no position
  uint64_t *rng_b, *rng_e;           // the locus as rows [b, e) of the sorted keys
  uint64_t *pieces, *piece_off;      // n_loci + 1: pieces of kVcfSplit rows, and their scan
  uint64_t n_pieces;
  const uint32_t* allowed;           // words: the columns the first variant names
  uint32_t* counts;                  // n_loci x n_samples
  uint32_t* foreign;                 // set when a counted row holds a het bit outside `allowed`
};
size_t vcf_tmp_bytes(uint64_t n_lines);
size_t vcf_count_tmp_bytes(uint64_t n_loci);
hipError_t launch_vcf_classify(const VcfArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_vcf_compact(const VcfArgs& a, hipStream_t s);
hipError_t launch_vcf_parse(const VcfArgs& a, hipStream_t s);
hipError_t launch_vcf_runs_scan(const VcfArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_vcf_runs(const VcfArgs& a, hipStream_t s);
hipError_t launch_vcf_sort(const VcfArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_vcf_flags(const VcfArgs& a, hipStream_t s);
// out[0]: the line of the kept row whose key is key[d]
hipError_t launch_vcf_last_of(const VcfArgs& a, uint64_t d, uint32_t* out, hipStream_t s);
hipError_t launch_vcf_ranges(const VcfArgs& a, const VcfCountArgs& c, void* tmp, size_t tmp_bytes,
                             hipStream_t s);
hipError_t launch_vcf_count(const VcfArgs& a, const VcfCountArgs& c, hipStream_t s);

// ---------------------------------------------------------------------------
// exclude_from_fasta, fasta2tab: FASTA records of a resident text
// (fastarec.hip; genome_tools.py:377-391, magot_smallfuncs.py:21-29;
// magot_fastarec_*)
// ---------------------------------------------------------------------------
// A line whose first byte is '>' is a header and opens a record; every other
// line adds its bytes, less the LF and a CR before it, to the open record.  No
// pass walks a sequence line: a line's payload is known from its two ends.
constexpr uint32_t kFaMaxName = 1024;  // bytes of a name one lane hashes; a longer name declines
constexpr uint32_t kFaPiece = 4096;    // bytes of a sequence line one lane slot of the reflow copies
constexpr uint64_t kFaMaxLines = (1ull << 31) - 1;
constexpr int kFaGroup = 16;           // pieces per wave of the reflow's copy
static_assert((kFaPiece & (kFaPiece - 1)) == 0, "a power of two");
struct FaArgs {
  // the text (readable to the next multiple of 16 and 16 more) and its line index:
  // ix.pos[k] is where line k starts
  TextIndexArgs ix;
  unsigned long long* status;  // min of (line << 8 | MAGOT_FASTAREC_* reason); ~0 when clean
  // per line, ix.n_lines + 1 of each (the last entry of the first three 0, of the scans the total)
  uint64_t *hdr, *pay, *pcs;              // 1 for a header; payload bytes; pieces of kFaPiece
  uint64_t *rec_of, *pay_pre, *pcs_pre;   // their exclusive scans
  // per record (header line), n_rec of each where nothing else is said
  uint64_t n_rec;
  uint32_t* hdr_line;    // n_rec + 1, the last entry n_lines
  uint64_t *name_off, *word_off, *hash, *word_hash, *seq_len;
  uint32_t *name_len, *word_len, *no_word;
  uint64_t *ne, *ne_pos;  // n_rec + 1: 1 where the sequence is not empty, and the scan
  // the records with a sequence, compacted in file order, then sorted by the masked hash
  uint32_t hash_bits;
  uint64_t n_ne;
  uint64_t *skey, *skey_sorted;
  uint32_t *sval, *sval_sorted;
  uint64_t *head, *head_pos;  // a run head's own position, else 0; their running maximum
  uint64_t *is_first, *kpos;  // n_rec + 1: 1 on a key's first record, and the scan
  uint32_t* last_of;          // on a key's first record: its last record
  // per key in first-seen order
  uint64_t n_keys;
  uint64_t* k_hash;
  uint32_t *k_first, *k_last, *k_no_word;
};
struct FaMemberArgs {  // the exclusion names: one blob, m + 1 offsets
  uint64_t m;
  const uint8_t* blob;
  const uint64_t* off;
  uint64_t *lkey, *lkey_sorted;  // m: the masked hashes
  uint32_t *lidx, *lidx_sorted;
  uint32_t first_word;           // compare each key's first word, not its name
  uint8_t* keep;                 // n_keys: 0 where the compared name is in the list
};
enum { kFaStyleFasta = 0, kFaStyleTab = 1 };
struct FaRenderArgs {
  uint64_t n_out;        // records to print
  const uint32_t* recs;  // n_out, each below n_rec, in output order
  uint32_t style;
  uint64_t *olen, *obase;  // n_out + 1: bytes of each printed record, the last 0; the scan
  uint64_t *pcnt, *pbase;  // n_out + 1: 1 + its sequence pieces, the last 0; the scan
  uint64_t n_pieces;
  uint64_t *p_src, *p_dst;  // n_pieces: in the text, in `out`
  uint32_t* p_len;
  uint8_t* out;  // obase[n_out] bytes, 16-byte aligned
};
size_t fa_tmp_bytes(uint64_t n);  // of every pass over at most n lines, records, names or pieces
hipError_t launch_fa_lines(const FaArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_fa_names(const FaArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_fa_sort(const FaArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_fa_keys(const FaArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_fa_rows(const FaArgs& a, hipStream_t s);
hipError_t launch_fa_member(const FaArgs& a, const FaMemberArgs& m, void* tmp, size_t tmp_bytes,
                            hipStream_t s);
hipError_t launch_fa_render_sizes(const FaArgs& a, const FaRenderArgs& r, void* tmp,
                                  size_t tmp_bytes, hipStream_t s);
hipError_t launch_fa_render(const FaArgs& a, const FaRenderArgs& r, hipStream_t s);

// ---------------------------------------------------------------------------
// replace_names: words of a resident text renamed from a table (rename.hip;
// genome_tools.py:431-446; magot_rename_*)
// ---------------------------------------------------------------------------
// A key is a name and the one-byte delimiter d.  A field is what lies between
// two ds of a line; the name that rewrites it is the one of lowest rank among
// the names that are suffixes of it.  One lane per d walks left over at most the
// longest name of the table, whatever the field's length.
constexpr uint32_t kRnMaxName = 256;  // bytes of a name; a longer one never reaches the device
constexpr uint32_t kRnPiece = 4096;   // bytes of an unchanged run one lane slot of the copy takes
constexpr uint32_t kRnNoKey = 0xffffffffu;
constexpr uint64_t kRnMaxKeys = 1ull << 30;   // the slots are numbered in 32 bits
constexpr uint64_t kRnMaxBlob = 1ull << 32;   // a value is one piece: its length fits 32 bits
struct alignas(16) RnSlot {  // of the open-addressing table; 16 bytes, one load
  uint64_t hash;  // the name's masked matching hash
  uint32_t key;   // kRnNoKey: empty
  uint32_t len;
};
struct RnArgs {
  // the text (readable to the next multiple of 16 and 16 more) and the index of
  // its ds: ix.byte is d, ix.pos[j] the offset of field end j; the LFs are
  // counted beside them
  TextIndexArgs ix;
  uint32_t hash_bits;
  // the table: n_keys distinct names, each of 1..kRnMaxName bytes without d
  uint64_t n_keys;
  const uint8_t* names;
  const uint64_t *name_off, *val_off;  // n_keys + 1 each
  uint64_t val_base;     // the value blob's first byte, counted from `text` (as readable as it)
  const uint32_t* rank;  // n_keys: the key's place in the dict order in use
  uint64_t* key_hash;    // n_keys: the masked hash, from the name's last byte to its first
  uint32_t* claim;       // cap: the key that took the slot (compare-and-swap), kRnNoKey
  RnSlot* slots;         // cap
  uint64_t cap;          // a power of two, at least 4 * n_keys
  uint32_t slot_shift;   // 64 - log2(cap)
  uint32_t max_len;      // the longest name
  uint64_t len_mask[kRnMaxName / 64];  // bit l - 1: a name of l bytes exists
  unsigned long long* status;  // min of the MAGOT_RENAME_* reasons met, ~0 when clean
  // per field end (a d of the text), n_fields of each where nothing else is said
  uint64_t n_fields;
  uint32_t* f_key;            // the key that rewrites the field, kRnNoKey
  uint64_t *f_hit, *f_hpos;   // n_fields + 1: 1 where there is one, the last entry 0; the scan
  // per hit in text order
  uint64_t n_hits;
  uint64_t* h_end;            // its d
  uint32_t* h_key;
  uint64_t *h_delta, *h_dsum;  // n_hits + 1: value less name in bytes (mod 2^64), the last 0; the scan
  uint64_t *h_pcnt, *h_pbase;  // n_hits + 2: pieces of the run before the hit and 1 for its value;
                               // entry n_hits: the run behind the last hit; then 0; the scan
};
struct RnRenderArgs {
  uint64_t n_pieces;
  uint64_t *p_src, *p_dst;  // n_pieces: from `text`, in `out`
  uint32_t* p_len;
  uint8_t* out;       // out_bytes, 16-byte aligned
  uint64_t out_bytes;  // n + h_dsum[n_hits]
};
hipError_t launch_rn_table(const RnArgs& a, hipStream_t s);
hipError_t launch_rn_match(const RnArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_rn_layout(const RnArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_rn_render(const RnArgs& a, const RnRenderArgs& r, hipStream_t s);

// ---------------------------------------------------------------------------
// tab2fasta, repeatmasker2augustushints: column cuts of a resident text
// (tabcut.hip; magot_smallfuncs.py:12-18, genome_tools.py:449-454;
// magot_tabcut_*)
// ---------------------------------------------------------------------------
// A cut is a small program run on every line: a line with fewer than `need`
// TABs is skipped or reported, every other line prints the program's items, a
// literal of the blob or the source bytes of the fields a..b (inner TABs
// included).  A field ends at one of the line's first `need` TABs; field
// `need` ends at the next TAB when the line has one, else at the line's end
// less the LF and less one CR before it.  No pass reads a field's bytes: a
// line's cost is a search in the TAB offsets and the items.
constexpr uint32_t kTcPiece = 4096;  // bytes of an item one lane slot of the copy takes
constexpr uint32_t kTcMaxItems = 8;
constexpr uint64_t kTcMaxLines = (1ull << 31) - 1;
constexpr int kTcGroup = 16;         // pieces per wave of the copy
constexpr uint32_t kTcShortLine = 1;  // the status word's reason
enum { kTcLiteral = 0, kTcFields = 1 };              // TcItem::kind (MAGOT_TABCUT_ITEM_*)
enum { kTcShortSkip = 0, kTcShortError = 1 };        // TcArgs::short_mode (MAGOT_TABCUT_SHORT_*)
enum { kTcSkipped = 0, kTcKept = 1, kTcShort = 2 };  // a line's verdict (MAGOT_TABCUT_LINE_*)
struct TcItem {
  uint32_t kind;
  uint32_t a, b;  // a literal: offset and length in the blob; fields: a <= b <= need
};
struct TcArgs {
  // the text (readable to the next multiple of 16 and 16 more) and its two
  // indexes: ix.pos[k] is where line k starts, tx.pos[j] the offset of TAB j
  // (tx counts nothing itself: its blk and pre are ix's blk2 and pre2)
  TextIndexArgs ix, tx;
  uint64_t n_tabs;
  uint32_t need, short_mode, n_items;
  TcItem items[kTcMaxItems];
  uint64_t lit_base;  // the literal blob's first byte, counted from `text` (as readable as it)
  unsigned long long* status;  // [0]: the stray-CR check's word; [1]: min of (line << 8 |
                               // kTcShortLine) over the short lines of error mode; ~0 when clean
  unsigned long long* n_kept;  // the lines with the verdict kTcKept
  // per line, ix.n_lines + 1 of each (the last entry of olen and pcnt 0, of the scans the total)
  uint8_t* verdict;
  uint64_t* tab0;           // the line's first TAB in tx.pos (n_tabs where none follows)
  uint64_t *olen, *obase;   // bytes the line prints; the scan
  uint64_t *pcnt, *pbase;   // its pieces of at most kTcPiece bytes, none for an empty item; the scan
};
struct TcRenderArgs {
  uint64_t n_pieces;
  uint64_t *p_src, *p_dst;  // n_pieces: from `text`, in `out`
  uint32_t* p_len;
  uint8_t* out;        // out_bytes, 16-byte aligned
  uint64_t out_bytes;  // obase[n_lines]
};
hipError_t launch_tc_rows(const TcArgs& a, hipStream_t s);
hipError_t launch_tc_layout(const TcArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_tc_pieces(const TcArgs& a, const TcRenderArgs& r, hipStream_t s);
hipError_t launch_tc_copy(const TcArgs& a, const TcRenderArgs& r, hipStream_t s);

// ---------------------------------------------------------------------------
// write_gff's text from a table of rows (gffwrite.hip; magot.h: magot_gffrow).
// Pass 1, one lane per row: the eight tabs of the row's source line, its score
// and phase classified, the output line's exact length.  A scan of the lengths.
// Pass 3, one wave per kGwGroup consecutive rows: every row's segments staged
// in LDS (a segment is a run of the text or blob, or a few bytes made up in
// LDS: the integers, the score, the literals), then the lanes dealt over the
// 16-byte chunks of the group's contiguous output range.
// ---------------------------------------------------------------------------
constexpr int kGwGroup = 32;      // rows per wave
constexpr int kGwThreads = 256;   // threads of a workgroup (4 waves)
constexpr uint32_t kGwMaxHead = 1u << 20;  // a line's eighth tab lies within so many bytes
constexpr uint32_t kGwMaxRef = 1u << 28;   // bytes of a referenced name
struct GwAux {            // per row, from pass 1
  uint32_t tab[8];        // the tabs of the source line, counted from line_off
  uint32_t int_off, int_len;    // score: integer digits without leading zeros, from line_off
  uint32_t frac_off, frac_len;  // score: fraction digits without trailing zeros
  uint32_t flags;         // kGwScoreNum, kGwScoreNeg, kGwPhase
  uint32_t pad[3];
};
constexpr uint32_t kGwScoreNum = 1, kGwScoreNeg = 2, kGwPhase = 4;
struct GwArgs {
  const uint8_t* text;  // n bytes
  uint64_t n;
  const uint8_t* blob;  // blob_len bytes: reference n + k is its byte k
  uint64_t blob_len;
  const magot_gffrow* rows;
  uint64_t n_rows;
  GwAux* aux;           // n_rows
  uint64_t* len;        // n_rows + 1: bytes of each output line, the last entry 0
  uint64_t* off;        // n_rows + 1: their exclusive scan
  unsigned long long* status;  // min of (row << 8 | MAGOT_GFFWRITE_* reason), ~0 when clean
};
hipError_t launch_gw_size(const GwArgs& a, hipStream_t s);
hipError_t launch_gw_render(const GwArgs& a, uint8_t* out, hipStream_t s);

// Standard genetic code (genome.py:795-802) as a 64-byte table indexed
// c0 + 4*c1 + 16*c2 with A=0, C=1, G=2, T=3.
void standard_lut(uint8_t out[64]);

// ---------------------------------------------------------------------------
// Errors
// ---------------------------------------------------------------------------
void set_error(const std::string& msg);

}  // namespace magot

// magot_mask_plan's result (maskplan.cpp), read by magot_mask_create (abi_mask.hip)
struct magot_maskplan {
  uint32_t flags = 0;
  std::vector<uint64_t> contig_lens;
  std::vector<magot_mask_interval> rows;  // pieces of at most kMaskPiece bases, in GFF order
};

// magot_overlap_plan's result (overlapplan.cpp): one row per line of each file
struct magot_ovtable {
  std::vector<uint8_t> flag;   // 1: more than 6 tabs
  std::vector<uint32_t> seq;   // dense seqid of the first file; kOvNoSeq: unknown, or no flag
  std::vector<int64_t> c0, c1; // int(x[3]), int(x[4]); 0 where they were not read
  std::vector<uint64_t> off, len;  // the line's place in its buffer, its LF included
};
struct magot_ovplan {
  magot_ovtable t[2];
  uint32_t n_seq = 0;
};

#define MAGOT_HIP_TRY(expr)                                                     \
  do {                                                                           \
    hipError_t e_ = (expr);                                                      \
    if (e_ != hipSuccess) {                                                      \
      ::magot::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));     \
      return MAGOT_ERR_HIP;                                                      \
    }                                                                            \
  } while (0)
