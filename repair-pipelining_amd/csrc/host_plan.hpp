// host_plan.hpp -- what the host-memory batches of host_pipe.cpp decide before they enqueue
// anything: the runs of a stripe's used slots, the copies that move them,
// the chunks and column slices a batch is cut into, the depth of the buffer ring, and the split
// of a batch over a device list.
//
// No HIP header and no other unit of the engine: the plans run -- and are tested -- on the CPU
// (tests/native/host_plan_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace ecx {

// Consecutive used slots that are also consecutive in host memory.
struct Run {
    int slot0;     // first host slot
    int compact0;  // first compact (device) slot
    int len;       // slots in the run
};
std::vector<Run> runs_of(const std::vector<int> &slots, int64_t slot_stride, int64_t nbytes);

// A maximal progression of equal runs -- runs i..j of one length, `ds` host slots and `dc` compact
// slots apart (both 0 for a lone run): the 3D copies of plan_copies and of the column slices.
struct Segment {
    size_t i, j;
    int64_t ds, dc;
};
std::vector<Segment> progressions_of(const std::vector<Run> &runs);

// One copy of a chunk of stripes (plan_copies has the three kinds).
struct Copy {
    int64_t host_off, dev_off;      // the copy's first byte in the chunk's first stripe
    int64_t width;                  // bytes per row
    int64_t rows;                   // rows per stripe
    int64_t host_pitch, dev_pitch;  // between a stripe's rows (folded: continuing across stripes)
    bool three_d;                   // rows of one stripe, then the next stripe a stripe stride on
};
// The copies that move `runs` of every stripe of a chunk between host stripes `stripe_stride`
// apart (slots `slot_stride` apart) and device stripes `per` apart (slots nbytes apart).
std::vector<Copy> plan_copies(const std::vector<Run> &runs, int64_t stripe_stride, int64_t slot_stride, int64_t per,
                              int64_t nbytes);

// Units (stripes) per chunk, the chunk count and the depth of the buffer ring, for units that each
// send `up_per` bytes up in `ncopies` copies per chunk.
struct Chunking {
    int64_t chunk, nchunks;
    int nb;
};
Chunking chunking_of(int64_t up_per, size_t ncopies, int64_t units, int64_t host_chunk, int host_buffers);

// The chunking and copy plan of one host batch (run_host_batch; run_host_check_batch, whose only
// output is one verdict byte per stripe: outputs == false).  A batch whose stripes all fit one
// chunk but carry far more than a chunk of input (config 4 with 1 MiB sub-chunks: one 3.5 GiB
// stripe per call) is cut into column slices instead -- bytes [c0, c0 + slice) of every slot, the
// map being bytewise -- so its H2D, kernel and D2H still overlap, the way the reference's repair
// pipelining slices a block (PipelineUtil.kt:13-28).
struct Plan {
    std::vector<Run> rin, rout;
    std::vector<Copy> cin, cout;
    std::vector<Segment> sin, sout;  // the runs' progressions, for column slices
    int64_t in_per = 0, out_per = 0, chunk = 1, nchunks = 0;
    int64_t slice = 0, nslices = 1;  // column slices (slice 0: whole slots)
    int nb = 1;
};
Plan make_plan(const std::vector<int> &ins, const std::vector<int> &outs, int64_t in_stripe_stride,
               int64_t in_slot_stride, int64_t out_stripe_stride, int64_t out_slot_stride, int64_t nstripes,
               int64_t nbytes, bool outputs, int64_t host_chunk, int host_buffers);

// The plan of a pattern set decoded in place (run_host_mixed_batch): a set's buffer keeps all n
// slots of a unit, nbytes apart, so the runs are not compacted and only the copies are sparse --
// the up slots go H2D, the down slots come back.  Chunks are sized by the bytes that go up.
struct HostMixedPlan {
    std::vector<Copy> cin, cout;
    int64_t per = 0;  // a unit on the device: [slot][nbytes], every slot
    int64_t chunk = 1, nchunks = 0;
    int nb = 1;
};
HostMixedPlan make_mixed_plan(const std::vector<int> &up, const std::vector<int> &down, int64_t stripe_stride,
                              int64_t slot_stride, int n, int64_t units, int64_t nbytes, int64_t host_chunk,
                              int host_buffers);

// The plan of a pattern set run out of place (run_host_map_mixed_batch, the Clay repair with a
// list per stripe): a set's input buffer keeps all n_in slots of a stripe and its output buffer
// all n_out, nbytes apart -- the set's plan addresses slots by their index -- so, as in the
// in-place plan, the runs are not compacted.  The set's input slots go H2D; every output slot
// comes back for every stripe (the part a stripe's own list does not write as zeros, which the
// pipeline puts there).  Chunks are sized by the bytes that go up.
struct HostMapMixedPlan {
    std::vector<Copy> cin, cout;
    int64_t in_per = 0, out_per = 0;  // a stripe on the device: [slot][nbytes], every slot
    int64_t chunk = 1, nchunks = 0;
    int nb = 1;
};
HostMapMixedPlan make_map_mixed_plan(const std::vector<int> &ins, const std::vector<int> &outs, int64_t in_stripe_stride,
                                     int64_t in_slot_stride, int n_in, int64_t out_stripe_stride,
                                     int64_t out_slot_stride, int n_out, int64_t nstripes, int64_t nbytes,
                                     int64_t host_chunk, int host_buffers);

// How run_host_batch moves a batch (ecx_map_host_plan, include/ecx_tune.h): stripes per chunk, the
// chunk count, device buffer sets in flight, and per chunk the H2D / D2H copies, the most rows per
// stripe one copy moves (> 1 where runs are folded or copied in 3D) and how many copies are 3D.
struct HostBatchPlan {
    int64_t chunk = 0, nchunks = 0;
    int buffers = 0;
    int64_t h2d_copies = 0, h2d_rows = 0, d2h_copies = 0, d2h_rows = 0, h2d_3d = 0, d2h_3d = 0;
    int64_t slices = 0;  // column slices of a one-chunk batch (1: whole slots)
};
// make_plan (with outputs) folded into those counts; all zero for a batch of no stripes or bytes.
HostBatchPlan host_batch_plan(const std::vector<int> &ins, const std::vector<int> &outs, int64_t in_stripe_stride,
                              int64_t in_slot_stride, int64_t out_stripe_stride, int64_t out_slot_stride,
                              int64_t nstripes, int64_t nbytes, int64_t host_chunk, int host_buffers);

// Part j of `parts` contiguous stripe ranges of nstripes, the remainder on the first parts (the
// rule of shard_stripes, __init__.py; the split of the _devices batches).
void stripe_range(int64_t nstripes, int parts, int j, int64_t *begin, int64_t *end);

// Fewer stripes than device entries (one or two huge stripes): the _devices batches split the
// bytes of every slot instead, in 4 KiB units -- the map is bytewise -- so every entry's link
// still carries a share.  The number of those units, or 0 for a batch that splits by stripes.
constexpr int64_t kColUnit = 4096;
int64_t column_units(int64_t nstripes, int ndev, int64_t nbytes);

}  // namespace ecx
