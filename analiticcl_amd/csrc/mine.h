// mine.h -- anx_mine_confusables: what mine_capi.cpp (host: argument checks, chunking, texts, the merged table) asks of mine.hip (device:
// edit scripts, site keys, the histogram, the site list).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "engine.h"
#include "host_model.h"

namespace anx {

// One distinct site text of a chunk as the device hands it back: where its representative lies (the host builds the text from the
// caller's strings) and the sums over every site with the same code points.
struct MineRow {
  uint32_t pair;   // chunk-relative
  uint32_t pos;    // a_pos | a_len << 8 | b_pos << 16 | b_len << 24 (code points; a side has at most 64 on the device)
  uint32_t meta;   // left context | right context << 4 (code points) | first << 8 | last << 9
  uint32_t _pad;
  uint64_t count, sites;
};
static_assert(sizeof(MineRow) == 32, "MineRow is 32 bytes");

constexpr uint32_t MINE_MAX_CONTEXT = 8;
constexpr int MINE_NCTR = 8;  // anx_debug_mine_stats

// The site records of a chunk, kept on the device until the merged table -- and with it every site's final pattern index -- is known.
struct MineChunk;
void mine_chunk_free(MineChunk*);
size_t mine_chunk_sites(const MineChunk*);  // sites the device found (host pairs have none there)

// One chunk of at most PAIRS_CHUNK pairs on dl's device.  rows: the chunk's distinct site texts (index = the pattern index its site
// records carry); host_pairs: the pairs the lane memory could not hold or whose script had an unexpected shape, ascending -- they have
// no sites on the device.  counts: per-pair counts or nullptr (1 each).  stats[4] += hash runs that held more than one text,
// stats[5] += pairs handed back for their script's shape.  *chunk: nullptr when keep_sites is false or there are no sites.
int mine_chunk_run(const DeviceLexicon* dl, const PairSpan* a, const PairSpan* b, const uint32_t* counts, size_t n, uint32_t context, bool anchors,
                   bool keep_sites, MineChunk** chunk, std::vector<MineRow>& rows, std::vector<uint32_t>& host_pairs, uint64_t* stats,
                   uint64_t* bytes_up, uint64_t* bytes_down, std::string& err);
// The chunk's site list in (pair, position) order with pattern = remap[chunk pattern index] and pair = pair_base + chunk pair:
// out[mine_chunk_sites()], off[n + 1] (chunk-relative).
int mine_chunk_emit(MineChunk* chunk, const uint32_t* remap, size_t nrows, uint32_t pair_base, anx_mine_site* out, uint32_t* off, uint64_t* bytes_down,
                    std::string& err);

}  // namespace anx
