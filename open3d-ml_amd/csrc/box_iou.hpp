// box_iou.hpp — rotated-rectangle overlap shared by the NMS mask kernel
// (nms.hip), the pairwise IoU kernel (box_iou.hip) and the host IoU
// (box_iou_host.cpp).  († Open3D IoUImpl, restated: Open3D is un-vendored, so
// the contract below is positional and parity-unpinned, as for NMS; the same
// float32 algorithm is oracle/o3d_oracle.c orc_bev_iou.)
//
// A rectangle is (x_min, y_min, x_max, y_max, yaw), rotated about its centre.
// The overlap polygon of two rectangles is the set of proper edge crossings
// plus the corners of either that lie inside the other, ordered by angle
// about their mean; its area is the shoelace sum.
//
//   BEV row (cx, cy, w, l, ry) -> (cx-w/2, cy-l/2, cx+w/2, cy+l/2, ry),
//       IoU = inter / max(sa + sb - inter, 1e-8)
//   3D row (x, y, z, w, h, l, ry), camera frame, y the bottom face:
//       footprint (x, z, w, l, ry); height overlap of [y-h, y];
//       ov = area * height, v = w*h*l, IoU = ov / max(va + vb - ov, 1e-8)
//
// Disjoint boxes give exactly 0.0f.  Every function is safe for any float
// input (NaN, inf, zero or negative sizes): loops are bounded by constants and
// the polygon never holds more than kMaxPoly points.
#pragma once

#include <cmath>

#if defined(__HIPCC__) || defined(__HIP__)
#define O3DML_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define O3DML_HD inline
#endif

namespace o3dml {

constexpr float kIouEps = 1e-8f;
// Two convex quadrilaterals: each of the 4 edges of one crosses the boundary
// of the other at most twice (8 crossings), plus at most 4 + 4 contained
// corners.  Appends past this are dropped (reachable only by non-finite or
// degenerate input).
constexpr int kMaxPoly = 16;

struct P2 {
    float x, y;
};

O3DML_HD float cross3(P2 p1, P2 p2, P2 p0) {
    return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

O3DML_HD bool rect_cross(P2 p1, P2 p2, P2 q1, P2 q2) {
    return fminf(p1.x, p2.x) <= fmaxf(q1.x, q2.x) && fminf(q1.x, q2.x) <= fmaxf(p1.x, p2.x) &&
           fminf(p1.y, p2.y) <= fmaxf(q1.y, q2.y) && fminf(q1.y, q2.y) <= fmaxf(p1.y, p2.y);
}

O3DML_HD bool in_box(const float* b, P2 p) {
    const float margin = 1e-5f;
    const float cx = (b[0] + b[2]) * 0.5f, cy = (b[1] + b[3]) * 0.5f;
    const float c = cosf(-b[4]), s = sinf(-b[4]);
    const float rx = (p.x - cx) * c + (p.y - cy) * s + cx;
    const float ry = -(p.x - cx) * s + (p.y - cy) * c + cy;
    return rx > b[0] - margin && rx < b[2] + margin && ry > b[1] - margin && ry < b[3] + margin;
}

// Segment p0-p1 against q0-q1; writes the crossing point.
O3DML_HD bool seg_cross(P2 p1, P2 p0, P2 q1, P2 q0, P2& ans) {
    if (!rect_cross(p0, p1, q0, q1)) return false;
    const float s1 = cross3(q0, p1, p0), s2 = cross3(p1, q1, p0);
    const float s3 = cross3(p0, q1, q0), s4 = cross3(q1, p1, q0);
    if (!(s1 * s2 > 0.f && s3 * s4 > 0.f)) return false;
    const float s5 = cross3(q1, p1, p0);
    if (fabsf(s5 - s1) > kIouEps) {
        ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float d = a0 * b1 - a1 * b0;
        ans.x = (b0 * c1 - b1 * c0) / d;
        ans.y = (a1 * c0 - a0 * c1) / d;
    }
    return true;
}

O3DML_HD void box_corners(const float* b, P2* c) {
    const float cx = (b[0] + b[2]) * 0.5f, cy = (b[1] + b[3]) * 0.5f;
    const float co = cosf(b[4]), si = sinf(b[4]);
    const float xs[4] = {b[0], b[2], b[2], b[0]}, ys[4] = {b[1], b[1], b[3], b[3]};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c[k].x = (xs[k] - cx) * co + (ys[k] - cy) * si + cx;
        c[k].y = -(xs[k] - cx) * si + (ys[k] - cy) * co + cy;
    }
    c[4] = c[0];
}

// Area of the overlap polygon of two (x1,y1,x2,y2,yaw) rectangles; exactly 0
// when fewer than three polygon points are found.
O3DML_HD float rect_overlap_area(const float* a, const float* b) {
    P2 ca[5], cb[5];
    P2 pts[kMaxPoly];  // <= 8 edge crossings + 8 contained corners
    box_corners(a, ca);
    box_corners(b, cb);
    int cnt = 0;
    P2 ctr{0.f, 0.f};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            P2 x;
            if (cnt < kMaxPoly && seg_cross(ca[i + 1], ca[i], cb[j + 1], cb[j], x)) {
                ctr.x += x.x;
                ctr.y += x.y;
                pts[cnt++] = x;
            }
        }
    for (int k = 0; k < 4; ++k) {
        if (cnt < kMaxPoly && in_box(a, cb[k])) {
            ctr.x += cb[k].x;
            ctr.y += cb[k].y;
            pts[cnt++] = cb[k];
        }
        if (cnt < kMaxPoly && in_box(b, ca[k])) {
            ctr.x += ca[k].x;
            ctr.y += ca[k].y;
            pts[cnt++] = ca[k];
        }
    }
    float area = 0.f;
    if (cnt > 2) {
        ctr.x /= cnt;
        ctr.y /= cnt;
        float ang[kMaxPoly];
        for (int k = 0; k < cnt; ++k) ang[k] = atan2f(pts[k].y - ctr.y, pts[k].x - ctr.x);
        for (int j = 0; j < cnt - 1; ++j)  // bubble sort, ascending angle
            for (int i = 0; i < cnt - j - 1; ++i)
                if (ang[i] > ang[i + 1]) {
                    const P2 tp = pts[i];
                    pts[i] = pts[i + 1];
                    pts[i + 1] = tp;
                    const float ta = ang[i];
                    ang[i] = ang[i + 1];
                    ang[i + 1] = ta;
                }
        for (int k = 0; k < cnt - 1; ++k) {
            const float ux = pts[k].x - pts[0].x, uy = pts[k].y - pts[0].y;
            const float vx = pts[k + 1].x - pts[0].x, vy = pts[k + 1].y - pts[0].y;
            area += ux * vy - uy * vx;
        }
    }
    return fabsf(area) * 0.5f;
}

// IoU of two (x1,y1,x2,y2,yaw) rectangles (the NMS box layout).
O3DML_HD float bev_iou(const float* a, const float* b) {
    const float inter = rect_overlap_area(a, b);
    const float sa = (a[2] - a[0]) * (a[3] - a[1]);
    const float sb = (b[2] - b[0]) * (b[3] - b[1]);
    return inter / fmaxf(sa + sb - inter, kIouEps);
}

// (cx, cy, w, l, ry) -> (x1, y1, x2, y2, ry)
O3DML_HD void centre_to_rect(float cx, float cy, float w, float l, float ry, float* r) {
    r[0] = cx - w / 2;
    r[1] = cy - l / 2;
    r[2] = cx + w / 2;
    r[3] = cy + l / 2;
    r[4] = ry;
}

enum BoxIouMode { kIouBev = 0, kIou3d = 1 };

O3DML_HD int box_iou_row_width(int mode) { return mode == kIou3d ? 7 : 5; }

// One (row of boxes_a, row of boxes_b) pair in `mode`'s row layout.
O3DML_HD float box_iou_pair(const float* a, const float* b, int mode) {
    float ra[5], rb[5];
    if (mode == kIou3d) {
        centre_to_rect(a[0], a[2], a[3], a[5], a[6], ra);
        centre_to_rect(b[0], b[2], b[3], b[5], b[6], rb);
        const float area = rect_overlap_area(ra, rb);
        const float height = fmaxf(fminf(a[1], b[1]) - fmaxf(a[1] - a[4], b[1] - b[4]), 0.f);
        const float ov = area * height;
        const float va = a[3] * a[4] * a[5], vb = b[3] * b[4] * b[5];
        return ov / fmaxf(va + vb - ov, kIouEps);
    }
    centre_to_rect(a[0], a[1], a[2], a[3], a[4], ra);
    centre_to_rect(b[0], b[1], b[2], b[3], b[4], rb);
    return bev_iou(ra, rb);
}

}  // namespace o3dml
