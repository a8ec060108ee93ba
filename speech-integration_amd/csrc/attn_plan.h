// The work plan of the attention backward for packed rows (ABI v7): its format, written down once.
// A plan is an array of int32 words, built on the HOST by ssi_attn_plan_build (attention_mfma.hip) and copied to the device by the caller; the
// first PLAN_HEADER_WORDS words are also what a launch needs on the host (ssi_attn_varlen_bwd_plan's host_plan_header).  Behind the header:
//   dK/dV items: PLAN_W_N_DKV_ITEMS x PlanDkvItem at word PLAN_W_DKV_OFF, heaviest first           (attn_bwd_dkv2_kernel<true>: one workgroup per item and kv head)
//   reduce list: PLAN_W_N_REDUCE x PlanReduceEntry at word PLAN_W_REDUCE_OFF: the 256-key chunks that were split over the query heads
//                                                                                                   (attn_dkv_plan_reduce_kernel)
//   dQ groups  : PLAN_W_N_DQ_GROUPS groups of PLAN_W_DQ_GROUP_WORDS words each at word PLAN_W_DQ_OFF: a PlanDqGroupHead, then PlanDqItem
//                slots up to the longest group's count, zero-filled                                 (attn_bwd_dq2_kernel<0, true>: one persistent workgroup per group and kv head)
// The kernels read items and entries as int4 (one per PlanDqItem / PlanDqGroupHead, two per PlanDkvItem / PlanReduceEntry); ssi/attn_plan.py
// names the words it decodes after this file.
#pragma once
#include <stdint.h>
#include "../../include/ssi_hip.h"

enum PlanWord {
    PLAN_W_MAGIC = 0,
    PLAN_W_N_DKV_ITEMS,
    PLAN_W_DKV_OFF,         // word offset of the dK/dV items
    PLAN_W_N_DQ_GROUPS,
    PLAN_W_DQ_OFF,          // word offset of the dQ groups
    PLAN_W_DQ_GROUP_WORDS,  // words per dQ group (fixed stride)
    PLAN_W_BATCH,
    PLAN_W_SEQ,
    PLAN_W_N_HEADS,
    PLAN_W_N_KV,
    PLAN_W_WORDS,           // total words
    PLAN_W_N_DOCS,
    PLAN_W_LSE_BEYOND,      // 1e30f: the "log-sum-exp" of a query that belongs to another document, P = 0 (read on the device by attn_bwd_dkv2_kernel<true>)
    PLAN_W_N_REDUCE,
    PLAN_W_REDUCE_OFF,      // word offset of the reduce list
    PLAN_W_N_SLOTS,         // fp32 partial slots of the split chunks: workspace = slots x n_kv x PLAN_SLOT_BYTES
    PLAN_HEADER_WORDS
};
static_assert(PLAN_HEADER_WORDS == SSI_ATTN_PLAN_HEADER, "plan header");

constexpr int32_t PLAN_MAGIC = 0x53534950;  // "SSIP"
constexpr int DKV2_MAX_STEPS = 2048;        // tiles per workgroup of attn_bwd_dkv2_kernel = (S / 32) * rep at most: S <= 16384 at rep = 4 (its tile table in LDS)
constexpr int PLAN_CHUNK_KEYS = 256;        // keys of a dK/dV item
constexpr int64_t PLAN_SLOT_BYTES = PLAN_CHUNK_KEYS * 128 * (int64_t)sizeof(float);  // per kv head: [256 keys][dK 64 | dV 64] fp32

struct PlanDkvItem { int32_t b, k0, dstart, dend, head0, heads, pslot /* partial slot or -1 */, pad; };
struct PlanReduceEntry { int32_t b, k0, dstart, dend, slot0, slots, pad[2]; };
struct PlanDqGroupHead { int32_t n_items, load, pad[2]; };
struct PlanDqItem { int32_t b, q0, dstart, dend; };
constexpr int PLAN_ITEM_WORDS = 8, PLAN_DQ_ITEM_WORDS = 4;
static_assert(sizeof(PlanDkvItem) == 4 * PLAN_ITEM_WORDS && sizeof(PlanReduceEntry) == 4 * PLAN_ITEM_WORDS, "two int4");
static_assert(sizeof(PlanDqGroupHead) == 4 * PLAN_DQ_ITEM_WORDS && sizeof(PlanDqItem) == 4 * PLAN_DQ_ITEM_WORDS, "one int4");
