// pcl_rules.h -- the rules the photon-writing sweeps share, each stated once (pcl_surface.hip, pcl_source.hip).  Device code only,
// included behind pcl_sweep.h and pcl_device.h.  Every helper is forced inline and does its arithmetic with the __d*_rn intrinsics
// in the order include/physicl_hip.h writes it out; physicl_amd/light.py holds the numpy helper of each rule.  A rule is a helper
// here only if every kernel that calls it stays the same machine code (tools/compare_unit_asm.py); pcl_surface.hip lists the rest.
#ifndef PCL_RULES_H
#define PCL_RULES_H

namespace pcl_rules {

// x.y of two vectors is always (x0*y0 + x1*y1) + x2*y2
__device__ __forceinline__ double dot3(const double *x, const double *y) {
    return __dadd_rn(__dadd_rn(__dmul_rn(x[0], y[0]), __dmul_rn(x[1], y[1])), __dmul_rn(x[2], y[2]));
}

// The head of a sweep whose ballots need every lane of a wave inside the loop: whole waves run the same number of trips.
__device__ __forceinline__ int64_t first_slot() { return (int64_t)blockIdx.x * pcl_sweep::kBlock + threadIdx.x; }
__device__ __forceinline__ int64_t grid_stride() { return (int64_t)gridDim.x * pcl_sweep::kBlock; }
__device__ __forceinline__ int64_t whole_waves(int64_t N) { return (N + 63) / 64 * 64; }

// The id of slot i: its place in the array if the store keeps one, id_base + i otherwise.
__device__ __forceinline__ uint64_t id_of(const int64_t *ids, int64_t id_base, int64_t i) {
    return (uint64_t)(ids ? ids[i] : id_base + i);
}

// The uniforms of a Philox block -- the call stays at its site, where its counter word can be read: u53(w0, w1) [and u53(w2, w3)].
__device__ __forceinline__ double first_u53(pcl_u32x4 w) { return pcl_u53(w.x, w.y); }
__device__ __forceinline__ void pair_u53(pcl_u32x4 w, double *u_a, double *u_b) {
    *u_a = pcl_u53(w.x, w.y);
    *u_b = pcl_u53(w.z, w.w);
}

// (rho cos psi, rho sin psi) of psi = (u*2)*pi: the scatter step's angle.
__device__ __forceinline__ void azimuth(double rho, double u, double *rc, double *rs) {
    double sn, cs;
    pcl_sincos_2pi(__dmul_rn(__dmul_rn(u, 2.0), PCL_PI), &sn, &cs);
    *rc = __dmul_rn(rho, cs);
    *rs = __dmul_rn(rho, sn);
}

// The sine to a cosine mu, s = sqrt((1 - mu)*(1 + mu)), about the azimuth of u_b: sc = s*cos psi, ss = s*sin psi.
__device__ __forceinline__ void polar(double mu, double u_b, double *sc, double *ss) {
    azimuth(__dsqrt_rn(__dmul_rn(__dsub_rn(1.0, mu), __dadd_rn(1.0, mu))), u_b, sc, ss);
}

// An orthonormal frame e1, e2 about the unit vector n (Duff et al. 2017, branch-free):  sg = copysign(1, n2);  aa = -1/(sg + n2);
//   bb = (n0*n1)*aa;  sn0 = sg*n0;  e1 = (1 + (sn0*n0)*aa, sg*bb, -sn0);  e2 = (bb, sg + (n1*n1)*aa, -n1)
__device__ __forceinline__ void frame(const double *n, double *e1, double *e2) {
    const double sg = copysign(1.0, n[2]);
    const double aa = __ddiv_rn(-1.0, __dadd_rn(sg, n[2]));
    const double bb = __dmul_rn(__dmul_rn(n[0], n[1]), aa), sn0 = __dmul_rn(sg, n[0]);
    e1[0] = __dadd_rn(1.0, __dmul_rn(__dmul_rn(sn0, n[0]), aa)); e1[1] = __dmul_rn(sg, bb); e1[2] = -sn0;
    e2[0] = bb; e2[1] = __dadd_rn(sg, __dmul_rn(__dmul_rn(n[1], n[1]), aa)); e2[2] = -n[1];
}

// One component of the direction (sc*e1 + ss*e2) + mu*axis.
__device__ __forceinline__ double turned(double sc, double ss, double mu, double e1, double e2, double axis) {
    return __dadd_rn(__dadd_rn(__dmul_rn(sc, e1), __dmul_rn(ss, e2)), __dmul_rn(mu, axis));
}

// law_mu for the closed-form laws: the cosine of the scattering angle of PCL_PHASE_ISOTROPIC, PCL_PHASE_HG (g) and PCL_PHASE_RAYLEIGH
// from u_a, in the lines include/physicl_hip.h writes out for pcl_step_phase_redirect -- Henyey-Greenstein by the closed inverse for
// |g| >= 1/2 and by the same inverse as a polynomial in g below it (no difference of ones), g == 0 the isotropic line; Rayleigh's
// 3/2 mu^2 part (one lane in four) draws the block (id_lo, id_hi, pass, 11).  A tabulated law, and any other kind, gets the isotropic
// line: its caller overwrites it.  k_phase_grid calls it; k_phase_redirect and k_phase_layered keep these lines written out (the call
// changes them).
__device__ __forceinline__ double law_mu(int law, double g, double u_a, uint64_t id, uint32_t pass, uint32_t k0, uint32_t k1) {
    double mu = __dsub_rn(1.0, __dmul_rn(2.0, u_a));                    // uniform on the sphere
    if (law == PCL_PHASE_HG && g != 0.0) {
        const double gg = __dmul_rn(g, g);
        if (fabs(g) < 0.5) {
            const double s = mu, gs = __dmul_rn(g, s), d = __dsub_rn(1.0, gs), s2 = __dmul_rn(s, s);
            const double p = __dadd_rn(__dsub_rn(__dmul_rn(0.5, __dadd_rn(s2, 3.0)), gs), __dmul_rn(gg, __dmul_rn(0.5, __dsub_rn(s2, 1.0))));
            mu = __ddiv_rn(__dsub_rn(__dmul_rn(g, p), s), __dmul_rn(d, d));
        } else {
            const double g2 = __dmul_rn(2.0, g);
            const double q = __ddiv_rn(__dsub_rn(1.0, gg), __dadd_rn(__dsub_rn(1.0, g), __dmul_rn(g2, u_a)));
            mu = __ddiv_rn(__dsub_rn(__dadd_rn(1.0, gg), __dmul_rn(q, q)), g2);
        }
        mu = fmin(fmax(mu, -1.0), 1.0);
    } else if (law == PCL_PHASE_RAYLEIGH) {
        const double s4 = __dmul_rn(u_a, 4.0), jq = floor(s4);
        const double gq = __dsub_rn(__dmul_rn(2.0, __dsub_rn(s4, jq)), 1.0);
        mu = gq;
        if (jq == 3.0) {
            const pcl_u32x4 wb = pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), pass, 11u, k0, k1);
            mu = copysign(fmax(fmax(fabs(gq), pcl_u53(wb.x, wb.y)), pcl_u53(wb.z, wb.w)), gq);
        }
    }
    return mu;
}

} // namespace pcl_rules

#endif // PCL_RULES_H
