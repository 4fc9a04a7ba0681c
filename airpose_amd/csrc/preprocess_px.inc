// One output pixel of the network's input contract, once, for stem.hip (libairpose_hip.so: preprocess_kernel behind
// ap_preprocess_crops) and synth_batch.hip (libairpose_grad.so: synth_crops_kernel behind apg_synth_crops).  Included inside each
// file's unnamed namespace.
//
// aerialpeople_crop.__getitem__ (copenet/src/copenet/dsets/aerialpeople.py:125-141,174) + resize_with_pad (utils/utils.py:214-235):
//   img = frame[:, :, ::-1] / 255 -> crop -> cv2.resize (float image: INTER_LINEAR, half-pixel centres, float
//   coefficients, border clamp) to int(scale*w) x int(scale*h), scale = 224 / max(h, w) -> zero padding to
//   224x224, centred -> CHW float -> Normalize(mean, std).   One thread per output pixel, all three channels.
// f: the image the crop is cut from (H x W x 3, uint8); crop: its y0, y1, x0, x1; out: its (3, 224, 224); scale_out, pad_out: its
// scale and (left, top).  Thread px == 0 writes scale and pad; a thread with px >= 224 * 224 writes no pixel.
// The products and sums below contract as stem.hip's build contracts them, whatever the including file's own -ffp-contract says:
// the two libraries must give the same bits for the same crop.
__device__ __forceinline__ void preprocess_px(const unsigned char* __restrict__ f, int W, int bgr, const int* __restrict__ crop,
                                              float* __restrict__ out, float* __restrict__ scale_out, int* __restrict__ pad_out,
                                              int px) {
#pragma clang fp contract(fast)
    const int y0 = crop[0], y1 = crop[1], x0 = crop[2], x1 = crop[3];
    const int h = y1 - y0, w = x1 - x0;
    const double scale = 224.0 / (double)(h > w ? h : w);
    const int dw = (int)(scale * w), dh = (int)(scale * h);
    const int pad_top = (224 - dh) / 2, pad_left = (224 - dw) / 2;
    if (px == 0) {
        scale_out[0] = (float)scale;
        pad_out[0] = pad_left;
        pad_out[1] = pad_top;
    }
    if (px >= 224 * 224) return;
    const int oy = px / 224, ox = px - oy * 224, dy = oy - pad_top, dx = ox - pad_left;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    float v[3] = {0.f, 0.f, 0.f};
    if (dy >= 0 && dy < dh && dx >= 0 && dx < dw) {
        // cv::resize, INTER_LINEAR: scale_x = 1 / (dw / w) in double, fx = (float)((dx + 0.5) * scale_x - 0.5)
        const double sxd = 1.0 / ((double)dw / (double)w), syd = 1.0 / ((double)dh / (double)h);
        float fx = (float)((dx + 0.5) * sxd - 0.5), fy = (float)((dy + 0.5) * syd - 0.5);
        int sx = (int)floorf(fx), sy = (int)floorf(fy);
        fx -= sx; fy -= sy;
        if (sx < 0) { fx = 0.f; sx = 0; }
        if (sx >= w - 1) { fx = 0.f; sx = w - 1; }
        if (sy < 0) { fy = 0.f; sy = 0; }
        if (sy >= h - 1) { fy = 0.f; sy = h - 1; }
        const int sx1 = sx + 1 < w ? sx + 1 : sx, sy1 = sy + 1 < h ? sy + 1 : sy;
        const unsigned char* p00 = f + ((size_t)(y0 + sy) * W + x0 + sx) * 3;
        const unsigned char* p01 = f + ((size_t)(y0 + sy) * W + x0 + sx1) * 3;
        const unsigned char* p10 = f + ((size_t)(y0 + sy1) * W + x0 + sx) * 3;
        const unsigned char* p11 = f + ((size_t)(y0 + sy1) * W + x0 + sx1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int cs = bgr ? 2 - c : c;
            const float a = p00[cs] / 255.f, b = p01[cs] / 255.f, cc = p10[cs] / 255.f, d = p11[cs] / 255.f;
            const float top = a * (1.f - fx) + b * fx, bot = cc * (1.f - fx) + d * fx;
            v[c] = top * (1.f - fy) + bot * fy;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[((size_t)c * 224 + oy) * 224 + ox] = (v[c] - mean[c]) / stdv[c];
}
