// The ring tiles with one accumulator column block per wave pair and the
// persistent form (k_conv3_ring PT = 1: each workgroup walks pixel tiles with
// the next tile's halo and first weights in flight during this tile's last
// chunk and epilogue), a second translation unit so the ring instantiations
// compile in two halves in parallel.  (A persistent 8 x 32 x 64 / 32-channel
// geometry spilled 200-500 B per lane around its epilogue and ran 1.2-1.4x
// slower than the plain one; measured persistent vs plain 8 x 32 x 64 / 64: 7-11 %
// faster on the 64-128-channel layers, tools/conv_bench.py --a16.)
#include "conv3_ring_kernel.h"
#include "unet_internal.h"

namespace unet {

IgemmTileRows conv3_ring_pt_tile_rows() {
  static const IgemmTile rows[] = {
      ring_tile<4, 128, 2, 2, 32, 2, 0>(83, 3),  // 4 waves (2 x 2), 64 x 64 per wave; 51 KB, 3 WG/CU
      ring_tile<8, 64, 8, 1, 64, 2, 0>(84, 1),   // 8 waves (8 x 1), 32 x 64 per wave; 114 KB, 1 WG/CU
  };
  return tile_rows(rows);
}

// persistent: the whole K per workgroup (no K split)
IgemmTileRows conv3_ring_persistent_tile_rows() {
  static const IgemmTile rows[] = {ring_tile<8, 64, 8, 1, 64, 2, 1>(88, 1)};
  return tile_rows(rows);
}

}  // namespace unet
