// Runs the entry points of a host-compiled copy of csrc/detect.hip (common.h's ADH_HOST_EMU_STREAM section: the dynamic LDS of
// nms_scan_kernel is a heap block of exactly `words` uint64, hipMemsetAsync is memset; the script format is stream_rt.h's).
// Calls, with their integers `i`, doubles `d` and buffers `b` in order:
//   0 adh_upsample_nearest_add  i: top_cs th tw lat_cs N H W C                        b: top lateral
//   1 adh_rpn_decode            i: cls_cs reg_cs N H W A stride_h stride_w  d: img_h img_w   b: cls reg base_anchors boxes logits
//   2 adh_nms_words             i: M
//   3 adh_nms_sorted            i: M                                  d: iou_threshold   b: boxes group mask_workspace keep
//   4 adh_roi_align_fpn         i: nlevels R C, then H W cs per level     d: scale per level  b: rois out, then f per level
//                               (adh_fpn_levels is filled from these; nlevels < 0: a null `levels`; levels past the buffers
//                               given keep a null f)
//   5 adh_box_postprocess       i: l_cs d_cs R NC                     d: score_thresh min_size
//                                                                     b: logits deltas props img_hw img boxes scores valid
#include "common.h"
#include "stream_rt.h"

static int64_t dispatch(const emu_call& c) {
    typedef int32_t i32;
    switch (c.fn) {
        case 0: return adh_upsample_nearest_add(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.f(1), c.I(3), c.I(4), c.I(5), c.I(6), c.I(7));
        case 1:
            return adh_rpn_decode(nullptr, c.f(0), c.I(0), c.f(1), c.I(1), c.I(2), c.I(3), c.I(4), c.I(5), c.I(6), c.I(7), c.f(2),
                                  (float)c.d[0], (float)c.d[1], c.f(3), c.f(4));
        case 2: return adh_nms_words(c.I(0));
        case 3: return adh_nms_sorted(nullptr, c.f(0), c.p<i32>(1), c.I(0), (float)c.d[0], c.p<void>(2), c.p<i32>(3));
        case 4: {
            if (c.I(0) < 0) return adh_roi_align_fpn(nullptr, nullptr, c.f(0), c.I(1), c.I(2), c.f(1));
            adh_fpn_levels L;
            memset(&L, 0, sizeof(L));
            L.nlevels = c.I(0);
            for (int l = 0; l < 4 && 3 + 3 * l + 2 < (int)c.i.size(); ++l) {
                L.H[l] = c.I(3 + 3 * l), L.W[l] = c.I(4 + 3 * l), L.cs[l] = c.I(5 + 3 * l);
                L.scale[l] = (float)c.d[l];
                if (2 + l < (int)c.ptr.size()) L.f[l] = c.f(2 + l);
            }
            return adh_roi_align_fpn(nullptr, &L, c.f(0), c.I(1), c.I(2), c.f(1));
        }
        case 5:
            return adh_box_postprocess(nullptr, c.f(0), c.I(0), c.f(1), c.I(1), c.f(2), c.f(3), c.p<i32>(4), c.I(2), c.I(3),
                                       (float)c.d[0], (float)c.d[1], c.f(5), c.f(6), c.p<i32>(7));
    }
    return -1000;
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
