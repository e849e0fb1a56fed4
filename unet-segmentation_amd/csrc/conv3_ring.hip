// k_conv3_ring tiles on 64- and 32-channel chunks with two accumulator column
// blocks per wave, and the ring family's fits (kernel: conv3_ring_kernel.h; the
// remaining tiles are instantiated in conv3_ring_pt.hip, a second translation
// unit that compiles in parallel).
#include "conv3_ring_kernel.h"

namespace unet {

// A sources bf16 (the plan's raw conv outputs with their consumer transform,
// normalised copies, padded dY, pooled maps, convT outputs); a transform only
// on source 0 (the second source of a concat is the convT output); no split
// operands (ring_tile's fits adds what depends on the geometry)
bool conv3_ring_fits(const IgemmArgs& a, const IgemmTile& t) {
  const Gather& g = a.a;
  const bool two = g.c_split < g.Cg, xtf = g.s[0].scale != nullptr;
  return a.bh != nullptr && a.bl == nullptr && a.N % t.bn == 0 && g.taps_h == 3 && g.taps_w == 3 && g.stride == 1 &&
         a.K == 9 * g.Cg && g.Cg % t.ch == 0 && g.c_split % t.ch == 0 && g.s[0].h16 &&
         (!two || (g.s[1].h16 && g.s[1].scale == nullptr)) && (!xtf || g.s[0].shift != nullptr);
}

IgemmTileRows conv3_ring_tile_rows() {
  static const IgemmTile rows[] = {
      ring_tile<8, 128, 4, 2, 64, 2, 0>(81, 1),  // 8 waves (4 x 2), 64 x 64 per wave; 138 KB, 1 WG/CU
      ring_tile<8, 64, 4, 1, 32, 2, 0>(82, 2),   // 4 waves (4 x 1), 64 x 64 per wave; 57 KB, 2 WG/CU
  };
  return tile_rows(rows);
}

}  // namespace unet
