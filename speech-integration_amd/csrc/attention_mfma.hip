// The MFMA flash attention (bf16, head_dim 64) as one translation unit: the kernels with their launches come in by kernel — attn_fwd.h,
// attn_bwd_dq.h, attn_bwd_dkv.h, in this order (attn_mfma.h says why they are not compiled apart, and holds the orientation and the shared device
// helpers) —; below them the host side: which shapes the kernels take, the backward's mode switches, the work plan for packed rows (format:
// attn_plan.h) and the backward dispatcher.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <vector>
#include "attn_mfma.h"
#include "attn_plan.h"
#include "attn_fwd.h"
#include "attn_bwd_dq.h"
#include "attn_bwd_dkv.h"

// Which backward kernels ssi_attn_bwd_mfma may take (ssi_set_attn_impl; process-global like ssi_set_impl).  The environment variables
// SSI_ATTN_DQ / SSI_ATTN_DKV give the INITIAL values, read once under C++ static initialisation — never on the launch path.
static int attn_env_mode(const char* name, int max_mode) {
    const char* s = getenv(name);
    const int v = (s && s[0] >= '0' && s[0] <= '9' && !s[1]) ? s[0] - '0' : 0;
    return v <= max_mode ? v : 0;
}
static std::atomic<int>& attn_mode(int which) {
    static std::atomic<int> modes[2] = {{attn_env_mode("SSI_ATTN_DQ", SSI_ATTN_MODE_NEW)}, {attn_env_mode("SSI_ATTN_DKV", SSI_ATTN_MODE_NO_HEAD_SPLIT)}};
    return modes[which];
}
extern "C" int ssi_set_attn_impl(int which, int mode) {
    if (which != SSI_ATTN_KERNEL_DQ && which != SSI_ATTN_KERNEL_DKV) return -1;
    const int max_mode = which == SSI_ATTN_KERNEL_DQ ? SSI_ATTN_MODE_NEW : SSI_ATTN_MODE_NO_HEAD_SPLIT;
    if (mode < 0 || mode > max_mode) return attn_mode(which).load(std::memory_order_relaxed);
    return attn_mode(which).exchange(mode, std::memory_order_relaxed);
}

bool ssi_attn_mfma_supported(int64_t ld, int64_t batch, int64_t seq, int n_heads, int n_kv, int head_dim, int dtype) {
    if (dtype != SSI_BF16 || head_dim != HD) return false;
    const int rep = n_heads / n_kv;
    if (rep != 1 && rep != 2 && rep != 4) return false;
    const int wg_rows = 32 * ANW / rep < 128 ? 128 : 32 * ANW / rep;  // query rows per forward workgroup; dK/dV: 128-key groups
    if (seq < wg_rows || seq % wg_rows != 0) return false;
    if (ld % 8 != 0 || batch <= 0) return false;
    if (batch * n_kv * (seq / 32) > (1LL << 30)) return false;
    return true;
}

// ---- work plan for packed rows (ABI v7; layout: attn_plan.h) -----------------------------------------------------------------------------
extern "C" int64_t ssi_attn_plan_words(int64_t batch, int64_t seq, int64_t n_docs) {
    if (batch <= 0 || seq <= 0 || n_docs <= 0) return 0;
    const int64_t dkv = batch * seq / PLAN_CHUNK_KEYS + 2 * n_docs, dq = batch * seq / 64 + 2 * n_docs;
    return PLAN_HEADER_WORDS + PLAN_ITEM_WORDS * 4 * dkv /* split 4 ways */ + PLAN_ITEM_WORDS * dkv /* reduce list */ +
           PLAN_DQ_ITEM_WORDS * (dq + 512 /* group headers */ + dq /* slack of the fixed group stride */);
}

// Returns the number of words written (> 0), 0 when the pipelined kernels do not take this batch (the caller then passes no plan and the
// round-1..3 kernels run), < 0 on a bad argument.
extern "C" int64_t ssi_attn_plan_build(const int32_t* host_doc_row, const int32_t* host_doc_start, const int32_t* host_doc_end, int64_t n_docs,
                                       int64_t batch, int64_t seq, int n_heads, int n_kv, int flags, int32_t* host_plan, int64_t plan_words) {
    if (!host_doc_row || !host_doc_start || !host_doc_end || !host_plan || n_docs <= 0 || batch <= 0 || seq <= 0 || n_heads <= 0 || n_kv <= 0) return -1;
    if (plan_words < ssi_attn_plan_words(batch, seq, n_docs)) return -1;
    const bool force = (flags & SSI_ATTN_PLAN_FORCE) != 0;
    if (n_heads != 4 * n_kv || seq % 128 != 0 || seq > (1 << 24)) return 0;  // the pipelined kernels: 4 query heads per kv head
    struct It { int32_t b, r0, ds, de, work, head0 = 0, heads = 4, pslot = -1; };
    std::vector<It> dkv, dq;
    std::vector<int64_t> covered((size_t)batch, 0);
    int64_t keys = 0;
    for (int64_t d = 0; d < n_docs; ++d) {
        const int32_t b = host_doc_row[d], ds = host_doc_start[d], de = host_doc_end[d];
        if (b < 0 || b >= batch || ds < 0 || de <= ds || de > seq) return -1;
        covered[(size_t)b] += de - ds;
        keys += de - ds;
        for (int32_t k0 = ds & ~31; k0 < de; k0 += PLAN_CHUNK_KEYS) {
            const int per_head = (de + 31) / 32 - k0 / 32;
            if (per_head * 4 + 8 > DKV2_MAX_STEPS) return 0;  // a document longer than the tile table
            dkv.push_back({b, k0, ds, de, per_head * 4});
        }
        for (int32_t q0 = ds & ~63; q0 < de; q0 += 64) dq.push_back({b, q0, ds, de, (q0 >> 6) - (ds >> 6) + 1});
    }
    for (int64_t b = 0; b < batch; ++b)
        if (covered[(size_t)b] != seq) return -1;  // the documents must tile every row (overlaps are the caller's bug; gaps are caught here)
    // stable sorts by work, heaviest first (ties keep document order: reproducible plans)
    auto by_work = [](const It& x, const It& y) { return x.work > y.work; };
    std::stable_sort(dq.begin(), dq.end(), by_work);
    // dK/dV is one workgroup per (item, kv head) and CU: a launch lasts at least as long as its heaviest item.  Items above the chip's share
    // per CU are split over the query heads (2 x 2 or 4 x 1 heads; fp32 partial sums, added by a reduction pass over those chunks only)
    int64_t total = 0;
    for (const It& it : dkv) total += it.work;
    const int64_t share = std::max<int64_t>(1, total * n_kv / 256), n_chunks = (int64_t)dkv.size();
    const bool split_all = (flags & SSI_ATTN_PLAN_SPLIT_ALL) != 0;
    const int64_t split_pct = 115;  // a chunk is split from 1.15 x the share on (measured: 80 / 60 / 45 % split more chunks and LOSE 2-10 %, LAB_NOTES round 5)
    std::vector<It> items, red;
    int32_t n_slots = 0;
    for (const It& it : dkv) {
        int ways = 1;
        if (split_all) ways = (it.r0 / PLAN_CHUNK_KEYS) % 2 ? 2 : 4;
        else if (it.work * 100 > share * split_pct && it.work > 32) ways = it.work * 100 > share * 2 * split_pct ? 4 : 2;
        if (ways == 1) { items.push_back(it); continue; }
        It r = it;
        r.pslot = n_slots, r.heads = ways;  // (reduce entry: first slot, slots)
        red.push_back(r);
        for (int w = 0; w < ways; ++w) {
            It part = it;
            part.heads = 4 / ways, part.head0 = w * (4 / ways), part.pslot = n_slots++, part.work = it.work / ways;
            items.push_back(part);
        }
    }
    std::stable_sort(items.begin(), items.end(), by_work);
    dkv.swap(items);
    if (!force) {
        // many short documents: an item has room for 256 keys (dK/dV) / 64 queries (dQ) whatever the document holds
        if (n_chunks * PLAN_CHUNK_KEYS > 2 * keys + 2048 || (int64_t)dq.size() * 64 > 2 * keys + 2048) return 0;
    }
    // dQ: groups of equal load for persistent workgroups, one round of the chip (256 workgroups over n_kv heads), longest processing time first
    const int fixed_cost = 6;  // an item's cost outside its tiles, in tiles (14 000 of ~2 400 cycles)
    int n_groups = (int)std::min<int64_t>((int64_t)dq.size(), std::max<int64_t>(1, 256 / n_kv));
    std::vector<std::vector<It>> groups((size_t)n_groups);
    std::vector<int64_t> load((size_t)n_groups, 0);
    for (const It& it : dq) {
        int g = 0;
        for (int j = 1; j < n_groups; ++j)
            if (load[(size_t)j] < load[(size_t)g]) g = j;
        groups[(size_t)g].push_back(it);
        load[(size_t)g] += it.work + fixed_cost;
    }
    size_t cap = 0;
    for (const auto& g : groups) cap = std::max(cap, g.size());
    const int64_t gstride = PLAN_DQ_ITEM_WORDS * (1 + (int64_t)cap);
    const int64_t dkv_off = PLAN_HEADER_WORDS, red_off = dkv_off + PLAN_ITEM_WORDS * (int64_t)dkv.size(), dq_off = red_off + PLAN_ITEM_WORDS * (int64_t)red.size();
    const int64_t words = dq_off + gstride * n_groups;
    if (words > plan_words) return -1;
    int32_t* hd = host_plan;
    for (int i = 0; i < PLAN_HEADER_WORDS; ++i) hd[i] = 0;
    hd[PLAN_W_MAGIC] = PLAN_MAGIC, hd[PLAN_W_N_DKV_ITEMS] = (int32_t)dkv.size(), hd[PLAN_W_DKV_OFF] = (int32_t)dkv_off;
    hd[PLAN_W_N_DQ_GROUPS] = n_groups, hd[PLAN_W_DQ_OFF] = (int32_t)dq_off, hd[PLAN_W_DQ_GROUP_WORDS] = (int32_t)gstride;
    hd[PLAN_W_BATCH] = (int32_t)batch, hd[PLAN_W_SEQ] = (int32_t)seq, hd[PLAN_W_N_HEADS] = n_heads, hd[PLAN_W_N_KV] = n_kv;
    hd[PLAN_W_WORDS] = (int32_t)words, hd[PLAN_W_N_DOCS] = (int32_t)n_docs;
    { const float big = 1e30f; memcpy(&hd[PLAN_W_LSE_BEYOND], &big, sizeof(float)); }
    hd[PLAN_W_N_REDUCE] = (int32_t)red.size(), hd[PLAN_W_REDUCE_OFF] = (int32_t)red_off, hd[PLAN_W_N_SLOTS] = n_slots;
    int32_t* w = host_plan + dkv_off;
    auto put = [&w](const auto& e) { memcpy(w, &e, sizeof(e)); w += sizeof(e) / sizeof(int32_t); };
    for (const It& it : dkv) put(PlanDkvItem{it.b, it.r0, it.ds, it.de, it.head0, it.heads, it.pslot, 0});
    for (const It& it : red) put(PlanReduceEntry{it.b, it.r0, it.ds, it.de, it.pslot, it.heads, {0, 0}});
    for (int g = 0; g < n_groups; ++g) {
        w = host_plan + dq_off + gstride * g;
        put(PlanDqGroupHead{(int32_t)groups[(size_t)g].size(), (int32_t)load[(size_t)g], {0, 0}});
        for (size_t i = 0; i < cap; ++i) {
            if (i < groups[(size_t)g].size()) { const It& it = groups[(size_t)g][i]; put(PlanDqItem{it.b, it.r0, it.ds, it.de}); }
            else put(PlanDqItem{0, 0, 0, 0});
        }
    }
    return words;
}

extern "C" int64_t ssi_attn_plan_workspace_bytes(const int32_t* host_plan_header) {
    if (!host_plan_header || host_plan_header[PLAN_W_MAGIC] != PLAN_MAGIC) return -1;
    return (int64_t)host_plan_header[PLAN_W_N_SLOTS] * host_plan_header[PLAN_W_N_KV] * PLAN_SLOT_BYTES;
}

static std::atomic<int> g_last_dispatch{0};
void ssi_attn_note_dispatch(int v) { g_last_dispatch.store(v, std::memory_order_relaxed); }
extern "C" int ssi_attn_last_dispatch(void) { return g_last_dispatch.load(std::memory_order_relaxed); }

// plan_dev: the plan in device memory, host_plan_header: its first SSI_ATTN_PLAN_HEADER words on the host (both NULL: no plan)
int ssi_attn_bwd_mfma(const void* qkv, int64_t ld, const void* out, const void* dout, const float* lse, void* dqkv, float* delta,
                      const int32_t* doc_start, const int32_t* doc_end, const float* rope, int64_t table_len, const int32_t* positions,
                      int64_t batch, int64_t seq, int n_heads, int n_kv, void* workspace, int64_t workspace_bytes, const int32_t* plan_dev,
                      const int32_t* host_plan_header, void* stream) {
    const int selq = attn_mode(SSI_ATTN_KERNEL_DQ).load(std::memory_order_relaxed);
    const int sel = attn_mode(SSI_ATTN_KERNEL_DKV).load(std::memory_order_relaxed);
    // packed rows with a plan: the document-aware forms of the pipelined kernels (mode OLD sends either kernel back to the round-1..3 one)
    const int32_t* ph = (plan_dev && host_plan_header) ? host_plan_header : nullptr;
    if (ph) {
        // (plain causal rows — no document arrays — take a plan whose documents are the rows themselves: the same work, dealt out by load)
        if (ph[PLAN_W_MAGIC] != PLAN_MAGIC || ph[PLAN_W_BATCH] != batch || ph[PLAN_W_SEQ] != seq || ph[PLAN_W_N_HEADS] != n_heads ||
            ph[PLAN_W_N_KV] != n_kv || n_heads / n_kv != 4 || ph[PLAN_W_N_DKV_ITEMS] <= 0 || ph[PLAN_W_N_DQ_GROUPS] <= 0 || (rope && table_len <= 0) ||
            ((!doc_start || !doc_end) && (ph[PLAN_W_N_DOCS] != batch || positions))) {
            ssi_set_error("ssi_attn_varlen_bwd_plan: the plan does not belong to this batch (magic %x, batch %d, seq %d, heads %d / %d)", ph[PLAN_W_MAGIC],
                          ph[PLAN_W_BATCH], ph[PLAN_W_SEQ], ph[PLAN_W_N_HEADS], ph[PLAN_W_N_KV]);
            return SSI_ERR_ARG;
        }
    }
    const AttnBwdArgs a{qkv, ld, out, dout, lse, dqkv, delta, doc_start, doc_end, rope, table_len, positions, batch, seq, n_heads, n_kv,
                           workspace, workspace_bytes, plan_dev, ph, (hipStream_t)stream};
    int used = 0;
    if (const int rc = attn_bwd_dq_launch(a, selq, &used)) return rc;
    if (const int rc = attn_bwd_dkv_launch(a, sel, &used)) return rc;
    ssi_attn_note_dispatch(used | 0x10000);  // bit 16: an MFMA backward ran
    return SSI_OK;
}

#ifdef ATTN_TRACE
extern "C" int ssi_debug_attn_trace(void* dst_host, int kernel) {  // debug build only: copy one kernel's table to the host
    return (int)hipMemcpyFromSymbol(dst_host, HIP_SYMBOL(g_attn_trace), sizeof(unsigned long long) * TRACE_MAX * 6,
                                    sizeof(unsigned long long) * TRACE_MAX * 6 * (size_t)kernel, hipMemcpyDeviceToHost);
}
#endif
