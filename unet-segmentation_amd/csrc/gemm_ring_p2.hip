// k_gemm_ring tiles 97-99 (see gemm_ring.hip: the tiles compile in three units)
#define GEMM_RING_PART 2
#include "gemm_ring.hip"
