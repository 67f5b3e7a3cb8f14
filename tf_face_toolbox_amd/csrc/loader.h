// loader.h -- host launchers of the input pipeline's GPU transform (loader.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

hipError_t k_preprocess_u8(const unsigned char* slots, float* out, int n, long slot_stride, int channels, int in_h, int in_w,
                           int crop_h, int crop_w, hipStream_t st);
hipError_t k_preprocess_u8_aug(const unsigned char* slots, float* out, int n, long slot_stride, int channels, int in_h, int in_w,
                               int crop_h, int crop_w, hipStream_t st);
size_t k_preprocess_u8_geo_ws_bytes(int n, int channels, int crop_h, int crop_w);
hipError_t k_preprocess_u8_geo(const unsigned char* slots, float* out, int n, long slot_stride, int channels, int in_h, int in_w,
                               int crop_h, int crop_w, const float* table, void* ws, hipStream_t st);
hipError_t k_preprocess_u8_align(const unsigned char* slots, float* out, int n, long slot_stride, int channels, int crop_h, int crop_w,
                                 hipStream_t st);
hipError_t k_pack_gather_slots(const unsigned char* rows, long num_rows, long row_stride, const int64_t* index,
                               const unsigned char* headers, unsigned char* slots, int n, long slot_stride, int cus, hipStream_t st);
