// ik_plan.cpp -- resize plans: the host half of resize_image's resampler.
//
// The weights, the choice of kernel variant and every table are computed without
// a device in ik_resize_plan.h (shared with the CPU model, ik_resize_model.cpp);
// this file caches plans and uploads their tables.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>

#include "ik_internal.h"
#include "ik_runtime.h"


namespace ik {
namespace {

std::mutex g_plan_mu;
// (device, W, H, C, iw, ih, x0, y0, nw, nh, filter, band height, flush): a crop of a
// resize and the whole resize to the crop's size are different plans
typedef std::array<int, 13> PlanKey;
std::map<PlanKey, ResizePlan*> g_plans;
// request -> plan (several requests can share one plan in g_plans)
typedef std::array<int, 12> FrontKey;
std::map<FrontKey, ResizePlan*> g_front;

template <typename T>
size_t put(std::vector<char>& blob, const std::vector<T>& v) {
    size_t off = (blob.size() + 255) & ~size_t(255);
    blob.resize(off + v.size() * sizeof(T));
    if (!v.empty()) std::memcpy(blob.data() + off, v.data(), v.size() * sizeof(T));
    return off;
}

}  // namespace

ResizePlan* build_resize_plan(int device, int W, int H, int C, int iw, int ih, int x0, int y0, int nw, int nh,
                              int filter, int n);

ResizePlan* get_resize_plan(int device, int W, int H, int C, int nw, int nh, int filter, int n) {
    return get_resize_plan_window(device, W, H, C, nw, nh, 0, 0, nw, nh, filter, n);
}

ResizePlan* get_resize_plan_window(int device, int W, int H, int C, int iw, int ih, int x0, int y0, int nw, int nh,
                                   int filter, int n) {
    // front cache on the request itself, so a repeated geometry costs a map
    // lookup, not a recomputation of the weights
    const FrontKey fkey = {device, W, H, C, iw, ih, x0, y0, nw, nh, filter, n};
    {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        auto it = g_front.find(fkey);
        if (it != g_front.end()) return it->second;
    }
    ResizePlan* p = build_resize_plan(device, W, H, C, iw, ih, x0, y0, nw, nh, filter, n);
    if (p) {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        g_front[fkey] = p;
    }
    return p;
}

ResizePlan* build_resize_plan(int device, int W, int H, int C, int iw, int ih, int x0, int y0, int nw, int nh,
                              int filter, int n) {
    ResizeTables t;
    resize_plan_head_window(W, H, C, iw, ih, x0, y0, nw, nh, filter, n, t);
    const PlanKey key = {device, W, H, C, iw, ih, x0, y0, nw, nh, filter, t.band_h, t.flush};
    std::lock_guard<std::mutex> lk(g_plan_mu);
    auto it = g_plans.find(key);
    if (it != g_plans.end()) return it->second;
    resize_plan_tables(t);
    const std::vector<int>&lx = t.lx, &cx = t.cx, &ly = t.ly, &cy = t.cy, &strips = t.strips, &bands = t.bands;
    const std::vector<int>&hdr = t.hdr, &band_step = t.band_step, &per_bands = t.per_bands;
    const std::vector<float>&wx = t.wx, &wy = t.wy, &sw = t.sw, &per_w = t.per_w;
    const std::vector<unsigned long long>& smask = t.smask;
    const int Tx = t.Tx, Ty = t.Ty;

    std::vector<char> blob;
    const size_t o_pw = put(blob, per_w), o_pb = put(blob, per_bands);
    const size_t o_ly = put(blob, ly), o_cy = put(blob, cy), o_wy = put(blob, wy);
    const size_t o_lx = put(blob, lx), o_cx = put(blob, cx), o_wx = put(blob, wx);
    const size_t o_st = put(blob, strips), o_bd = put(blob, bands);
    const size_t o_sh = put(blob, hdr), o_sm = put(blob, smask), o_sw = put(blob, sw), o_bst = put(blob, band_step);

    auto* p = new ResizePlan();
    p->W = W; p->H = H; p->C = C; p->nw = nw; p->nh = nh; p->filter = filter;
    p->iw = iw; p->ih = ih; p->x0 = x0; p->y0 = y0;
    p->slots = t.slots;
    p->rows = t.rows;
    p->weights_in_lds = t.weights_in_lds;
    p->flush = t.flush;
    p->NS = t.NS;
    p->NB = t.NB;
    p->per_A = t.per_A;
    p->per_R = t.per_R;
    p->table_bytes = blob.size();
    // upload on this thread's stream, synchronised there (copy_h2d_2d): done
    // before any stream launches with the plan, without a device-wide sync
    if (hipMalloc(&p->dev_tables, blob.size()) != hipSuccess) p->dev_tables = nullptr;
    if (!p->dev_tables ||
        copy_h2d_2d(static_cast<uint8_t*>(p->dev_tables), blob.size(), reinterpret_cast<const uint8_t*>(blob.data()),
                    blob.size(), blob.size(), 1,
                    thread_stream()) != IK_OK) {
        if (p->dev_tables) (void)hipFree(p->dev_tables);
        delete p;
        return nullptr;
    }
    mem_stat(kMemPlans, (int64_t)p->table_bytes);
    char* d = static_cast<char*>(p->dev_tables);
    ResizeArgs& a = p->args;
    a.W = W; a.H = H; a.C = C; a.nw = nw; a.nh = nh; a.row_bytes = W * C;
    a.ly = (const int*)(d + o_ly); a.ny = (const int*)(d + o_cy); a.wy = (const float*)(d + o_wy); a.Ty = Ty;
    a.lx = (const int*)(d + o_lx); a.nx = (const int*)(d + o_cx); a.wx = (const float*)(d + o_wx); a.Tx = Tx;
    a.strips = (const int*)(d + o_st); a.NS = p->NS;
    a.max_strip_cols = t.max_strip_cols;
    a.max_strip_weights = t.max_strip_weights;
    a.lds_pad = t.lds_pad;
    a.bands = (const int*)(d + o_bd); a.NB = p->NB;
    a.step_hdr = (const int*)(d + o_sh);
    a.step_mask = (const unsigned long long*)(d + o_sm);
    a.step_w = (const float*)(d + o_sw);
    a.band_step = (const int*)(d + o_bst);
    a.per_w = (const float*)(d + o_pw);
    a.per_bands = (const int*)(d + o_pb);
    a.per_base = t.per_base;
    a.NBp = t.NBp;
    a.tmp_col0 = t.col0;
    a.tmp_span = t.col_span;
    g_plans[key] = p;
    return p;
}

// ik_shutdown: every cached plan's device tables
void plans_shutdown() {
    std::lock_guard<std::mutex> lk(g_plan_mu);
    for (auto& kv : g_plans) {
        if (kv.second->dev_tables) {
            (void)hipFree(kv.second->dev_tables);
            mem_stat(kMemPlans, -(int64_t)kv.second->table_bytes);
        }
        delete kv.second;
    }
    g_plans.clear();
    g_front.clear();
}

}  // namespace ik
