// predict.hip -- the inter-frame predictor of a sequence (include/raht.h, "Inter-frame prediction").
// Row i of the current frame lies in the cell c = key[i] >> shift; its prediction is the mean of the reference rows of that cell,
// which are ONE run [lo, hi) of the reference's sorted keys: summed in float32 in row order from the run's first row, divided once
// by the run's length, 0 for an empty run. The order of the sum is part of the definition (a run holds at most 8^up <= 512 rows),
// so every implementation gives the same bits, and with shift = 0 the prediction is the co-located voxel's row exactly.
//
//   one launch, PR_TILE_ROWS rows per workgroup step:
//     resolve   one thread per row finds lo by binary search in the reference keys (an L2-resident table: 8 N' bytes) and hi by
//               another inside the 8^up rows behind lo; (lo, hi - lo) go to LDS, the rows with a run are counted.
//     move      the tile's elements flat. Matrices without padding (every row stride == D) move in 16-byte chunks that may
//               straddle rows (59 columns: 236-byte rows), X and Y nontemporal (touched once), the reference rows through the
//               cache (neighbouring voxels of a cell re-read them when shift > 0), two chunks per lane and round with their X
//               loads issued first; padded matrices move element by element.
//   Every row recomputes the mean of its run: no table of cell means is built (DESIGN.md 18 has the numbers).
// The device code lives in predict_device.h, which motion.hip shares.
#include "predict_device.h"

using namespace raht;

extern "C" {

int raht_predict(const uint64_t *keys_sorted, int64_t N, const uint64_t *ref_keys_sorted, int64_t N_ref, int shift, const float *C_ref,
                 int64_t ld_ref, const float *X, int64_t ldx, int D, int add, float *Y, int64_t ldy, int64_t *n_matched,
                 raht_stream_t stream)
{
    RAHT_RET(predict_check("raht_predict", keys_sorted, N, ref_keys_sorted, N_ref, shift, C_ref, ld_ref, X, ldx, D, add, Y, ldy));
    return predict_enqueue(keys_sorted, N, ref_keys_sorted, N_ref, shift, C_ref, ld_ref, X, ldx, D, add, Y, ldy, n_matched, SameKey(),
                           (hipStream_t)stream);
}

}  // extern "C"
