// LDS layout of the halo-patch bodies (3x3 stride 1): the patch image and the weight slabs.  Shared by the block-synchronous body
// (sp_patch.h, which describes the layout), by the wave-specialised body and by the pre-split weight images, whose slabs are
// WSTAGE bytes laid out like the LDS weight buffer (conv_ws.hip).
#pragma once
#include "sp_arith.h"

template <int NS, int TH, int WTN, int CS>
struct SpPatchLds {
  static constexpr int PP = (TH + 2) * 18;              // patch pixels
  // bytes per chunk image, padded to 64 mod 256: a 16-lane store group holds one pixel's granules of all CS chunks,
  // and chunk images a multiple of 128 bytes apart would put chunks 0 and 2 on the same banks
  static constexpr int CHUNK = PP * 32 + ((64 - (PP * 32) % 256) + 256) % 256;
  static constexpr int PPIECE = CS * CHUNK;             // per piece
  static constexpr int PATCH = sp_np(NS) * PPIECE;
  static constexpr int WPIECE = 16 * WTN * 64, WSTAGE = sp_np(NS) * WPIECE;
  static constexpr int BYTES = PATCH + 3 * WSTAGE;      // weight slabs: three buffers (fragments are read one slab ahead)
};
