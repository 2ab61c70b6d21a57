// The persistent decode launch of decode_block.hip, compiled a third time for the launch-tiled layout of a Llama-2-7B-shaped
// model's codes (codebook id 5 of quip_block_engine; quip_tile_codes / quip_tile_codes_view): see QUIP_BLOCK_TILED there.  Only the
// shipped E8P12 nibble kernel is instantiated here.
#define QUIP_BLOCK_TILED 1
#include "decode_block.hip"
