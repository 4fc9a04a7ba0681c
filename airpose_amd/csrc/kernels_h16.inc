// Launch interface of the kernel sources that are compiled once per 16-bit storage type (conv_igemm / conv_pipe / conv_slab /
// conv_lean / conv_pair / bottleneck2 / stem .hip).  No include guard: kernels.h includes this file inside namespace k_bf16 and
// inside namespace k_f16.  `kind` = K_F32 / K_BF16 (= "the 16-bit type of the set") / K_SPLIT; the k_f16 set carries the 16-bit
// kind only.
int ap_conv_cout_pad(void);
hipError_t ap_launch_conv(const ConvArgs& a, int kind, hipStream_t st);   // kind = AP_PREC_*: 0 fp32, 1 bf16, 2 split-bf16
// software-pipelined (LDS-DMA ring) variant; cfg: 0 = 256x128, 1 = 128x128, 2 = 128x64, 3 = 256x64
hipError_t ap_launch_conv_pipe(const ConvArgs& a, int kind, int cfg, hipStream_t st);

// stride-1 3x3 with the nine taps read from one LDS slab per 64-channel chunk (conv_slab.hip); bf16, 128x128 tiles
bool ap_conv_slab_supported(const ConvArgs& a, int kind);
hipError_t ap_launch_conv_slab(ConvArgs a, hipStream_t st);

// pointwise convolutions on three workgroups per CU (conv_lean.hip); bf16, 128x128 tiles, bit-identical to conv_pipe
bool ap_conv_lean_supported(const ConvArgs& a, int kind);
hipError_t ap_launch_conv_lean(ConvArgs a, hipStream_t st);

bool ap_conv_pair_supported(int P, int P2, int C3, int N1);
size_t ap_conv_pair_stream_bytes(int P, int P2, int C3, int N1);
// w3 [C3][P + P2], w1 [N1][C3]: K-contiguous bf16 rows as packed for the stand-alone kernels
hipError_t ap_launch_pair_pack(const void* w3, const void* w1, void* dst, int P, int P2, int C3, int N1, hipStream_t st);
hipError_t ap_launch_conv_pair(const PairArgs& a, int P, int P2, int C3, int N1, hipStream_t st);

// second cut: weights resident in LDS, x in registers (bottleneck2.hip); ds = 0 identity block, 1 first block of layer1
hipError_t ap_launch_bneck2(BneckArgs a, int ds, hipStream_t st);

// layer3 identity bottleneck, one image per workgroup, intermediates resident in LDS (block_img.hip)
size_t ap_block_img_stream_bytes(void);
hipError_t ap_launch_block_img_pack(const void* w1, const void* w2, const void* w3, void* dst, hipStream_t st);
hipError_t ap_launch_block_img(const BlkImgArgs& a, hipStream_t st);
// stride-1 3x3 of layer2 with half an image resident in LDS (conv_img3.hip)
bool ap_conv_img3_supported(int H, int W, int Cin, int Cout, int k, int stride, int pad);
size_t ap_conv_img3_stream_bytes(void);
hipError_t ap_launch_conv_img3_pack(const void* w2, void* dst, hipStream_t st);
hipError_t ap_launch_conv_img3(const ConvImg3Args& a, hipStream_t st);
// stride-2 3x3 of layer2.0 in polyphase form (conv_s2p.hip)
bool ap_conv_s2p_supported(int H, int W, int Cin, int Cout, int k, int stride, int pad);
size_t ap_conv_s2p_stream_bytes(void);
hipError_t ap_launch_conv_s2p_pack(const void* w2, void* dst, hipStream_t st);
hipError_t ap_launch_conv_s2p(const ConvS2pArgs& a, hipStream_t st);
// pointwise conv + BN (+ identity) + ReLU, 196-pixel x 256-channel tiles, one wave per SIMD (conv_pw.hip)
bool ap_conv_pw_supported(long M, int Cin, int Cout);
bool ap_conv_pw_ds_supported(const PwArgs& a);
bool ap_conv_pw_k3_supported(const PwArgs& a);
size_t ap_conv_pw_stream_bytes(int Cin, int Cout);
int ap_conv_pw_grid(long M, int Cout, int n_cu);
hipError_t ap_launch_conv_pw_pack(const void* w, void* dst, int Cin, int Cout, int wld, hipStream_t st);
hipError_t ap_launch_conv_pw(const PwArgs& a, hipStream_t st);

// conv 7x7/2 p3 (3->64) + BN + ReLU from NCHW fp32 into NHWC fp32 [N][112][112][64]: kind = K_F32 only (the exact fp32 FMA chain of
// the fp32 parity mode; defined in the bf16 set)
hipError_t ap_launch_stem_conv(const float* x_nchw, const float* w_k147x64, const float* scale, const float* shift,
                               void* y, int n_img, int kind, hipStream_t st);
// bf16 MFMA stem: images [0, n_split) come from x0, the rest from x1 (both views in one pass);
// w_packed: [64][AP_STEM_WLD] bf16, k' = r*32 + s*4 + c
hipError_t ap_launch_stem_conv_mfma(const float* x0, const float* x1, int n_split, const void* w_packed,
                                    const float* scale, const float* shift, void* y, int n_img, hipStream_t st);
// split-bf16 MFMA stem (bf16x2 mode): w_hi / w_lo: [64][AP_STEM_WLD] bf16 planes of the packed weights; y: split pairs
hipError_t ap_launch_stem_conv_mfma_split(const float* x0, const float* x1, int n_split, const void* w_hi, const void* w_lo,
                                          const float* scale, const float* shift, void* y, int n_img, hipStream_t st);
// fused split-bf16 stem + max-pool (bf16x2 mode): conv1 + bn1 + relu + maxpool, pooled split pairs [N][56][56][64]
hipError_t ap_launch_stem_pool_split(const float* x0, const float* x1, int n_split, const void* w_hi, const void* w_lo,
                                     const float* scale, const float* shift, void* y_pooled, int n_img, hipStream_t st);
// fused bf16 MFMA stem + maxpool: NCHW fp32 crops -> [N][56][56][64] bf16.  form 1: one workgroup per strip of two pooled rows;
// form 2: persistent workgroups, waves split into compute and load / pool roles (same bits)
hipError_t ap_launch_stem_pool(const float* x0, const float* x1, int n_split, const void* w_packed, const float* scale,
                                const float* shift, void* y_pooled, int n_img, int* range_flag, int form, hipStream_t st,
                                unsigned long long* dbg = nullptr);
// maxpool 3x3/2 p1: [N][112][112][64] -> [N][56][56][64]
hipError_t ap_launch_maxpool(const void* x, void* y, int n_img, int kind, int* range_flag, hipStream_t st);
// global 7x7 average: [N][49][C] T -> [N][C] fp32; range_flag (or NULL): host-mapped word set to 1 when a pooled value is not finite
hipError_t ap_launch_avgpool(const void* x, float* y, int n_img, int C, int kind, int* range_flag, hipStream_t st);

// crop + letter-box resize + /255 + normalise: uint8 HWC frames -> [n][3][224][224] fp32 (stem.hip)
hipError_t ap_launch_preprocess(const unsigned char* frames, size_t frame_stride, int n, int H, int W, int bgr,
                                const int* crop, float* out, float* scale_out, int* pad_out, hipStream_t st);
