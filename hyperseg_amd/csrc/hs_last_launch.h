// Device idioms of the forward's last launch that its sinks state once -- masks and confusion (hs_eval.hip), cross entropy with confusion
// (hs_validate.hip), overlay (hs_overlay.hip), confidence (hs_confidence.hip) -- in the two mappings the scoring kernels come in
// (DESIGN.md 3.11.4):
//   rows of four: one thread = 4 consecutive pixels of an output row (general and two-stage forms);
//   quads:        four consecutive lanes = one block of x, (row y, columns 2 q and 2 q + 1): a 2 x 4 output block (exact 2x) or a 4 x 8
//                 one (2x o 2x).
// Predicates stay with the caller: anything added here takes `vec` as a bool that its caller made -- from the entry's host-computed
// argument or from the address, as that kernel always did -- and "is there a mask", "is this lane live" are asked around the call.  The
// grid-stride loop headers stay in the kernels as well: their wave-uniform trip count is each kernel's visible contract.
// What is NOT here, and why (profiles/last_launch_helpers_isa.txt has the figures): the target loads, the mask stores, the counting tails
// and the quad picks of the scoring kernels.  Each of them, moved into a function of its own, changes the register allocation of the
// kernel it is inlined into (those kernels sit at 132-256 VGPRs), so they stay written out in the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hs_common.h"

namespace hs {

// The item of thread `threadIdx.x` in the pass of its workgroup that starts at `base`.  A surplus thread (live == false) shadows the
// image's last item: it computes (the callers' ballots and quad exchanges need every lane) and neither stores nor counts.
struct Item { bool live; int q, y; };
// rows of four: item = (row y, pixels 4 q .. 4 q + 3), wq items per row
__device__ __forceinline__ Item item_rows4(int base, int items, int wq) {
    const int e0 = base + (int)threadIdx.x;
    const bool live = e0 < items;
    const int e = live ? e0 : items - 1;
    return {live, e % wq, e / wq};
}
// quads: item = (x row y, x columns 2 q and 2 q + 1), wq items per row; the thread is lane threadIdx.x & 3 of the item's four
__device__ __forceinline__ Item item_quad(int base, int items, int wq) {
    const int e0 = base + (int)(threadIdx.x >> 2);
    const bool live = e0 < items;
    const int e = live ? e0 : items - 1;
    return {live, e % wq, e / wq};
}

}  // namespace hs
