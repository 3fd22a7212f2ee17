// rbf_block_plan.h -- the host arithmetic the dense-block stages share (hold, look-ahead, cut statistics, quality report, hold sweep, pan
// search, roll, views, digests): the checks of a block of packed frames, the split of a frame's pixels between a lane kernel and the per-pixel
// kernel behind it, the runs.  Pure host code, no HIP header: tests/c/block_plan_cases.cpp is built with a plain host compiler.
#pragma once
#include "../../include/rbf.h"

#include <cstdint>

static int fail(int code, const char *fmt, ...);                  // sets the thread's last-error text (rbf_host.h; a test brings its own)

// How an entry point's frames lie in memory (bytes), and what the entry point asks of that layout.
struct FrameLayout {
    uint32_t width, height;
    uint64_t row_pitch;
    uint32_t pixel_stride, sample_bytes;
    uint64_t frame_stride;           // 0: a single frame
};
struct LayoutRules {
    uint32_t samples = 1;            // samples of a pixel the entry point touches: the pixel stride has to hold them
    bool channels = false;           // `samples` is the caller's channel count: 1..4
    bool aligned = true;             // pixel stride, row pitch and frame stride are multiples of the sample size
    uint32_t min_frames = 0, max_frames = 0xFFFFFFFFu;
    uint32_t max_height = 0;         // 0: any
};

static int check_layout(const FrameLayout &l, uint32_t nframes, const LayoutRules &r)
{
    if (nframes < r.min_frames || nframes > r.max_frames)
        return fail(RBF_EINVAL, "frame count %u out of range %u..%u", nframes, r.min_frames, r.max_frames);
    if (l.width == 0 || l.height == 0) return fail(RBF_EINVAL, "empty frame %ux%u", l.width, l.height);
    if (r.max_height && l.height > r.max_height) return fail(RBF_ERANGE, "at most %u rows, got %u", r.max_height, l.height);
    if (l.sample_bytes != 1 && l.sample_bytes != 2) return fail(RBF_EINVAL, "sample_bytes must be 1 or 2, got %u", l.sample_bytes);
    if (r.channels && (r.samples == 0 || r.samples > 4)) return fail(RBF_EINVAL, "channels must be 1..4, got %u", r.samples);
    if (l.pixel_stride < r.samples * l.sample_bytes || (r.aligned && l.pixel_stride % l.sample_bytes))
        return fail(RBF_EINVAL, "pixel stride %u incompatible with %u sample(s) of %u bytes", l.pixel_stride, r.samples, l.sample_bytes);
    if (l.row_pitch < (uint64_t)l.width * l.pixel_stride || (r.aligned && l.row_pitch % l.sample_bytes))
        return fail(RBF_EINVAL, "row pitch %llu too small or misaligned", (unsigned long long)l.row_pitch);
    if (r.aligned && l.frame_stride % l.sample_bytes) return fail(RBF_EINVAL, "frame stride misaligned");
    return RBF_OK;
}

// A block of packed frames: width x height pixels of `channels` samples, nothing between the samples, the pixels or the rows.
struct PackedBlock {
    uint32_t width, height, channels, sample_bytes;
    uint64_t frame_stride;           // bytes
    uint32_t pixel() const { return channels * sample_bytes; }
    uint64_t n() const { return (uint64_t)width * height; }
    uint64_t frame_bytes() const { return n() * pixel(); }
    FrameLayout layout() const { return FrameLayout{width, height, (uint64_t)width * pixel(), pixel(), sample_bytes, frame_stride}; }
};

// A block is checked in two steps, because every entry has checks and no-op returns of its own between them.  First its shape: a
// frame that is not empty, 1..4 channels of 1 or 2 bytes, a stride that keeps the samples aligned.
static int check_block_shape(const PackedBlock &b, uint32_t nframes)
{
    LayoutRules rules;
    rules.samples = b.channels; rules.channels = true;
    return check_layout(b.layout(), nframes, rules);
}

// The frames do not overlap.  one_frame_any_stride: the entry does not look at the stride of a single frame.
static int check_frame_stride(uint64_t stride, uint64_t frame_bytes, uint32_t nframes, bool one_frame_any_stride)
{
    if (stride >= frame_bytes || (one_frame_any_stride && nframes <= 1)) return RBF_OK;
    return fail(RBF_EINVAL, "frame stride %llu smaller than a frame of %llu bytes", (unsigned long long)stride, (unsigned long long)frame_bytes);
}

// Then where a block of that shape lies: a base its samples are aligned at, frames that do not overlap.
static int check_block_at(const PackedBlock &b, uint32_t nframes, const void *base, bool one_frame_any_stride = false)
{
    if ((uintptr_t)base % b.sample_bytes) return fail(RBF_EINVAL, "frames misaligned for %u-byte samples", b.sample_bytes);
    return check_frame_stride(b.frame_stride, b.frame_bytes(), nframes, one_frame_any_stride);
}

// A lane kernel may run: every base (as an integer) and every stride given is a multiple of A, a power of two.  An entry that does not look
// at the stride of a single frame passes 0 for it.
template <class... U> static inline bool lanes_aligned(uint32_t A, U... bases_and_strides) { return (((uint64_t)bases_and_strides | ...) & (A - 1)) == 0; }

// The n pixels of a frame between a lane kernel and the per-pixel kernel behind it.  The lane kernel takes the whole units of unit_pixels
// pixels (none unless `vec`), units_per_workgroup to a workgroup; the per-pixel kernel the rest, tail_pixels_per_workgroup to a workgroup.
// Both write rows_per_workgroup rows of partial sums per workgroup into one array, the lane kernel's first; the kernels index them so.
struct LaneSplit {
    uint64_t units, first_px;        // whole units; the first pixel of the per-pixel kernel
    uint64_t bx_vec, bx_px;          // workgroups of the lane kernel and of the per-pixel kernel (0: not launched)
    uint64_t rows, tail_row_base;    // rows of the array; the per-pixel kernel's first
    bool fits() const { return bx_vec <= 0x7FFFFFFFull && bx_px <= 0x7FFFFFFFull; }       // both are a grid's x
};
static inline LaneSplit split_lanes(uint64_t n, uint32_t unit_pixels, uint32_t units_per_workgroup, uint32_t tail_pixels_per_workgroup,
                                    uint32_t rows_per_workgroup, bool vec)
{
    const uint64_t units = vec ? n / unit_pixels : 0, first_px = units * unit_pixels;
    const uint64_t bx_vec = (units + units_per_workgroup - 1) / units_per_workgroup;
    const uint64_t bx_px = (n - first_px + tail_pixels_per_workgroup - 1) / tail_pixels_per_workgroup;
    return LaneSplit{units, first_px, bx_vec, bx_px, (bx_vec + bx_px) * rows_per_workgroup, bx_vec * rows_per_workgroup};
}

// Frame 0 and every marked frame start a run (run_starts: a byte per frame, nullable; its first byte is not looked at).  Calls
// f(first, len) for every run in order until one returns non-zero, and returns that; which runs count is the caller's.
template <class F> static int for_each_run(const uint8_t *run_starts, uint32_t nframes, F &&f)
{
    for (uint32_t a = 0, b; a < nframes; a = b) {
        for (b = a + 1; b < nframes && !(run_starts && run_starts[b]);) ++b;
        if (int r = f(a, b - a)) return r;
    }
    return 0;
}
