R"GMMVI_DATA_TAPE(
// ---- reverse-mode gradients of a user-defined target summed over a data set (csrc/custom_target.hip puts this text behind the
// user's source, the whole text of the data mode (custom_target_data.inc and what stands in front of it) and the tape's number
// type (custom_target_tape.inc with GMMVI_TAPE_NO_KERNELS); contract: include/gmmvi_hip.h, "targets summed over a data set,
// differentiated on a tape") -----------------------------------------------------------------------------------------------------
// The text above defines gmmvi_user_row and gmmvi_user_prior, the source of the data mode, unchanged; the target is
//     lp(x) = prior(x) + s * sum over the row list of row(x, data[r]).
// A value call launches the data mode's own value kernels.  A gradient call launches the two kernels below per slab of tiles.
//
// gmmvi_data_tape_rows: grid (tiles of 64 samples in the slab, chunks), 64 threads = one wave, lane = sample (the tape's
// count() and tape() state in LDS are one wave's).  The wave owns rows_per_chunk consecutive positions of the row list; the row
// index is wave-uniform (gmmvi_data::row_at).  For each position in order the lane sets its record count to 0, records
// gmmvi_user_row<Var, Input> on the wave's tape, adds the value to its running sum and, if the count is within the capacity,
// walks the records back from the output node with seed 1, adding the adjoints of the inputs into its column of the wave's
// accumulator.  The same short tape serves every row.
// gmmvi_data_tape_rows_own: the same kernel for own batches: every lane reads the rows of its own batch (gmmvi_data::own_row_at,
// a per-lane pointer), so the record counts of one position differ from lane to lane by the row as well as by x.
// What keeps the adjoints of the previous row out of the current one: gmmvi_tape::push zeroes the adjoint slot of every record
// it writes, so each record the sweep reads carries an adjoint written since the current row began.  Records made after the output node are
// never visited: the sweep starts at the output's own record.
// gmmvi_data_tape_finish: grid (tiles in the slab), one wave, always launched.
//
// Scratch of wave w = chunk * tiles + tile: records rec[(w cap + r) * 64 + lane], adjoints adj[(w cap + r) * 64 + lane], and the
// gradient accumulator acc[(w D + i) * 64 + lane], a [D][64] image per wave: one read-modify-write of entry i by 64 lanes
// touches two cache lines (the output's [N, D] layout would touch 64).  After its last row the lane leaves its value sum in its
// adjoint slot 0, which no sweep needs any more: the finish kernel reads it from there.
// x is read straight from X[n, :] (lane stride D).
//
// Summation order (fixed; the only atomic is the integer maximum on *needed, so the same call gives the same bits): per lane the
// rows of a chunk in position order, values and adjoints alike (the adjoints of one row in sweep order: records from the output
// back to record 0); the chunks' partials in chunk-index order; then  s * sum;  then  + prior  for the value, and the prior's
// adjoints, from the prior recorded on the tape of chunk 0, added into the scaled accumulator in sweep order.
// A lane whose row term or prior makes more records than the capacity keeps evaluating values, sweeps nothing more, and raises
// *needed; its gradient is then incomplete and the host runs the call again at the needed capacity.

namespace gmmvi_data_tape {

using gmmvi_tape::AdjPtr;
using gmmvi_tape::Input;
using gmmvi_tape::Rec4;
using gmmvi_tape::RecPtr;
using gmmvi_tape::Var;

#define GMMVI_DATA_TAPE_FN __host__ __device__ __forceinline__

// The sweep is gmmvi_tape::sweep with the accumulator's stride: d out / d x[i] goes into acc[i * stride].
// One lane's share of a chunk: positions begin .. end - 1 of the row list, row_at(p) the floats of the row at position p.
// gmmvi_tape::tape() is set (stride, cap, D and the base the lane's rp / ap belong to).  -> the longest record count of a row.
template <class RowAt>
GMMVI_DATA_TAPE_FN int rows_lane(const float* x, int D, const float* params, int C, RowAt row_at, unsigned begin, unsigned end,
                                 RecPtr rp, AdjPtr ap, size_t stride, int cap, float* acc) {
    for (int i = 0; i < D; ++i) acc[(size_t)i * stride] = 0.f;
    float value = 0.f;
    int longest = 0;
    for (unsigned p = begin; p < end; ++p) {
        gmmvi_tape::count() = 0;
        const Var out = gmmvi_user_row<Var, Input>(Input{x}, D, row_at(p), C, params);
        value += out.v;
        const int made = gmmvi_tape::count();
        if (made > longest) longest = made;
        if (longest <= cap) gmmvi_tape::sweep(out, D, rp, ap, stride, x, acc, stride);
    }
    ap[0] = value;                                                   // the tape is done with: slot 0 carries the chunk's value sum
    return longest;
}

// One lane's finish.  ap / acc: the lane's adjoint slot 0 and accumulator entry 0 of chunk 0; chunk c lies c * adj_step /
// c * acc_step floats behind.  Writes *lp and, unless the prior overflows the tape, grad[0 .. D).  -> the prior's record count.
GMMVI_DATA_TAPE_FN int finish_lane(const float* x, int D, const float* params, int chunks, float scale, RecPtr rp, AdjPtr ap,
                                   size_t adj_step, float* acc, size_t acc_step, size_t stride, int cap, float* lp, float* grad) {
    float value = ap[0];
    for (int c = 1; c < chunks; ++c) value += ap[(size_t)c * adj_step];
    for (int i = 0; i < D; ++i) {
        float g = acc[(size_t)i * stride];
        for (int c = 1; c < chunks; ++c) g += acc[(size_t)c * acc_step + (size_t)i * stride];
        acc[(size_t)i * stride] = scale * g;
    }
    gmmvi_tape::count() = 0;
    const Var prior = gmmvi_user_prior<Var, Input>(Input{x}, D, params);
    const float scaled = scale * value;
    *lp = scaled + prior.v;
    const int made = gmmvi_tape::count();
    if (made > cap) return made;
    gmmvi_tape::sweep(prior, D, rp, ap, stride, x, acc, stride);
    for (int i = 0; i < D; ++i) grad[i] = acc[(size_t)i * stride];
    return made;
}

}  // namespace gmmvi_data_tape

#ifndef GMMVI_DATA_TAPE_NO_KERNELS
namespace gmmvi_data_tape {

// the body of gmmvi_data_tape_rows (OWN = false) and of gmmvi_data_tape_rows_own (OWN = true: the lane's own batch, its rows
// gmmvi_data::own_row_at from the origin of n, the sample's index in the call, whatever slab the launch serves)
template <bool OWN>
__device__ __forceinline__ void rows_kernel(int D, const float* params, const float* X, int N, const float* data,
                                            const gmmvi_data::RowList& l, int first_tile, void* rec, float* adj, float* acc, int cap,
                                            int* needed) {
    const int lane = (int)threadIdx.x;
    const size_t w = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const size_t tape_at = w * 64 * (size_t)cap;
    if (lane == 0) {
        gmmvi_tape::Tape& t = gmmvi_tape::tape();
        t.rec = (RecPtr)rec + tape_at;
        t.adj = (AdjPtr)adj + tape_at;
        t.stride = 64; t.cap = cap; t.D = D;
    }
    __syncthreads();
    const size_t n = ((size_t)first_tile + blockIdx.x) * 64 + lane;
    if (n >= (size_t)N) return;                                      // the lane's scratch columns stay unread
    const unsigned begin = blockIdx.y * l.rows_per_chunk;
    const unsigned end = l.length - begin < l.rows_per_chunk ? l.length : begin + l.rows_per_chunk;
    gmmvi_data::OwnOrigin o{};
    if constexpr (OWN) o = gmmvi_data::own_origin(n, l);
    const int longest = rows_lane(X + n * (size_t)D, D, params, l.C,
                                  [&](unsigned p) { return gmmvi_data::row_of<OWN>(data, l, o, p); }, begin, end,
                                  (RecPtr)rec + tape_at + lane, (AdjPtr)adj + tape_at + lane, 64, cap,
                                  acc + w * 64 * (size_t)D + lane);
    atomicMax(needed, longest);
}

}  // namespace gmmvi_data_tape

#define GMMVI_DATA_TAPE_ROWS_KERNEL(name, OWN)                                                                              \
    extern "C" __global__ __launch_bounds__(64) void name(int D, const float* __restrict__ params,                          \
                                                          const float* __restrict__ X, int N,                              \
                                                          const float* __restrict__ data, gmmvi_data::RowList l,           \
                                                          int first_tile, void* rec, float* adj, float* acc, int cap,      \
                                                          int* needed) {                                                   \
        gmmvi_data_tape::rows_kernel<OWN>(D, params, X, N, data, l, first_tile, rec, adj, acc, cap, needed);               \
    }
GMMVI_DATA_TAPE_ROWS_KERNEL(gmmvi_data_tape_rows, false)
GMMVI_DATA_TAPE_ROWS_KERNEL(gmmvi_data_tape_rows_own, true)
#undef GMMVI_DATA_TAPE_ROWS_KERNEL

extern "C" __global__ __launch_bounds__(64) void gmmvi_data_tape_finish(int D, const float* __restrict__ params,
                                                                         const float* __restrict__ X, int N, int chunks,
                                                                         float scale, int first_tile, void* rec, float* adj,
                                                                         float* acc, int cap, int* needed, float* lp, float* grad) {
    using namespace gmmvi_data_tape;
    const int lane = (int)threadIdx.x;
    const size_t tape_at = (size_t)blockIdx.x * 64 * (size_t)cap;    // chunk 0 of the tile
    if (lane == 0) {
        gmmvi_tape::Tape& t = gmmvi_tape::tape();
        t.rec = (RecPtr)rec + tape_at;
        t.adj = (AdjPtr)adj + tape_at;
        t.stride = 64; t.cap = cap; t.D = D;
    }
    __syncthreads();
    const size_t n = ((size_t)first_tile + blockIdx.x) * 64 + lane;
    if (n >= (size_t)N) return;
    const size_t tiles = gridDim.x;
    const int made = finish_lane(X + n * (size_t)D, D, params, chunks, scale, (RecPtr)rec + tape_at + lane,
                                 (AdjPtr)adj + tape_at + lane, tiles * 64 * (size_t)cap,
                                 acc + (size_t)blockIdx.x * 64 * (size_t)D + lane, tiles * 64 * (size_t)D, 64, cap, lp + n,
                                 grad + n * (size_t)D);
    atomicMax(needed, made);
}
#endif
#undef GMMVI_DATA_TAPE_FN
)GMMVI_DATA_TAPE"
