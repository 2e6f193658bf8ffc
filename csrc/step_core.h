// The decode step's per-row bookkeeping pieces shared by decode_prep / decode_advance
// (decode_step.hip) and the sampler's fused finish (sampling.hip): the next step's prep operands,
// their validation, the K/V write slot of a position, the clamped token and its embedding row.
#pragma once
#include "common.h"

namespace rt {

struct PrepArgs {   // next-step prep (all null: advance only)
  int64_t* slots;
  int64_t* offsets;
  uint16_t* res;
  const int* block_tables;
  const uint16_t* embed;
  int max_blocks, BS, H;
  int64_t vocab;
};

// what every launcher of a prep asks of its operands (the embedding row moves 16 B per lane)
inline bool prep_args_ok(const PrepArgs& pa) {
  return pa.slots != nullptr && pa.offsets != nullptr && pa.res != nullptr && pa.block_tables != nullptr &&
         pa.embed != nullptr && pa.H % 8 == 0 && pa.BS > 0 && pa.max_blocks > 0 && pa.vocab > 0;
}

// K/V write slot of position `pos` of row b = block_tables[b][pos / BS] * BS + pos % BS, in two
// steps so that a caller can put other loads between the block-table load and its use. Past the
// table (a turn's last step) the block resolves to 0: a slot that is never written.
RT_DEVICE int64_t kv_block(const PrepArgs& pa, int b, int64_t pos) {
  const int64_t bi = pos / pa.BS;
  return bi < pa.max_blocks ? pa.block_tables[(size_t)b * pa.max_blocks + bi] : 0;
}
RT_DEVICE int64_t kv_slot(const PrepArgs& pa, int64_t blk, int64_t pos) { return blk * pa.BS + pos % pa.BS; }

RT_DEVICE int64_t clamp_token(int64_t tok, int64_t vocab) { return tok < 0 ? 0 : (tok >= vocab ? vocab - 1 : tok); }

// 16-byte piece j of the clamped token's embedding row -> piece j of res[b, :]
RT_DEVICE void embed_piece(const PrepArgs& pa, int b, int64_t tok, int j) {
  const int row8 = pa.H / 8;
  reinterpret_cast<uint4*>(pa.res)[(size_t)b * row8 + j] =
      reinterpret_cast<const uint4*>(pa.embed)[(size_t)clamp_token(tok, pa.vocab) * row8 + j];
}

}  // namespace rt
