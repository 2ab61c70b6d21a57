// Host side shared by the persistent block engines: decode_block.hip, its QUIP_BLOCK_G8 build (decode_block_g8.hip) and
// decode_block_gqa.hip.  Each launcher keeps what differs: its n_layers bound, its codebook / QUIP_ENG_REP dispatch and
// the fields only its own argument struct has.
#pragma once
#include "launch.hip.h"
#include "quip_device.hip.h"

namespace quip {

// QUIP_ENG_REP: table mode of the E8P12 engines for A/B runs (24, 16; anything else: each engine's default), read once
inline int eng_rep_env() {
  static const int v = env_int("QUIP_ENG_REP", 4);
  return v;
}

// the fields that the kernel argument structs (Args = BlockArgs / GArgs, with their layer descriptor) share
template <class Args, class Layer>
Args block_args_of(const BlockEngineArgs& in) {
  Args a{};
  a.layers = reinterpret_cast<const Layer*>(in.layers);
  a.h_in = reinterpret_cast<const f16*>(in.h_in);
  a.h_out = reinterpret_cast<f16*>(in.h_out);
  a.pos = reinterpret_cast<const int64_t*>(in.pos);
  a.cos = in.cos; a.sin = in.sin;
  a.grid = reinterpret_cast<const uint64_t*>(in.grid);
  a.ws = reinterpret_cast<char*>(in.workspace);
  a.dbg = reinterpret_cast<uint64_t*>(in.dbg);
  a.n_layers = in.n_layers; a.max_len = in.max_len; a.dbg_layer = in.dbg_layer;
  a.rms_eps = in.rms_eps; a.attn_scale = in.attn_scale;
  return a;
}

}  // namespace quip
