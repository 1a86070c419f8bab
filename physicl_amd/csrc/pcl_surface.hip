// pcl_surface.hip -- the sweeps that rewrite photons: they re-direct them, absorb them, and re-emit the spent ones.
//
// A reflecting sphere (SurfaceReflectStep): the ground of a radial problem.  Photons whose last move took
// them into the sphere are put back: reflected at the point where the move met the sphere (specular, or cosine-weighted about
// the outward normal), or -- with an albedo below 1 -- absorbed there and left in the store at rest.  Nothing is removed.
//
// A translation unit of its own, linked into libphysicl_hip.so behind the other units on the public ABI: it does not see
// struct pcl_ctx and works through the public C ABI (include/physicl_hip.h) like any other host of the library; pcl_device.h is
// included for the Philox block, the 53-bit uniform and the project's sincos only.  The tuned kernels, their register budgets
// and the source hash the counter records are tied to (physicl_amd/build.py: csrc_sha) are not touched by anything here.  The
// scaffold it shares with the other units of its kind is pcl_sweep.h.
//
// The rules the six sweeps share are stated once in pcl_rules.h (pcl_source.hip includes it, too), where a helper leaves every
// kernel the same machine code (tools/compare_unit_asm.py).  These change a kernel and stay written out, each under a comment that
// names the rule: scattered / workable (dv != 0, 0 < o.o < inf), at_rest, dist2 and closed_bin (the radial layer, the bin of E),
// law_mu, source_mu and source_rho, park.  physicl_amd/light.py states every rule once for the numpy restatements, by these names.
//
//   k_surface_reflect<T>   one grid-stride sweep of the tiled slab: per slot r and dr of the three axes (48 B in fp64), widened
//                          to double; the shell sweep's q_now and q_prev against R*R decide who is hit; one ballot + popcount
//                          per wave for the two counters (LDS cells, flushed with 64-bit atomics).  Only lanes that are hit go
//                          on: they load v (and their id, if the store keeps an array of them), work the hit point and the new
//                          direction out in fp64 -- every operation rounded once, in the order written in
//                          include/physicl_hip.h -- and write r, v, dr, dv rounded once to the store's precision.
//
// Operation order (what light._surface_bounce restates with numpy; x.y of two vectors is always (x0*y0 + x1*y1) + x2*y2):
//   d = r - center, m = dr, p = d - m;  q_now = d.d, q_prev = p.p;  hit iff q_now < R2 <= q_prev < inf, a photon
//   a = m.m;  b = p.m;  cq = q_prev - R2;  disc = max(b*b - a*cq, 0);  t = cq / (sqrt(disc) - b)
//   x_k = p_k + t*m_k;  nrm_k = x_k / sqrt(x.x);  sa = sqrt(a);  w = (1 - t)*sa
//   absorbed (u_0 >= albedo):  r_k = center_k + x_k;  v_k = 0;  dr_k = x_k - p_k;  dv_k = 0 - v_old_k
//   specular:    mh_k = m_k / sa;  dn = mh.nrm;  dir_k = mh_k - (2*dn)*nrm_k
//   lambertian:  mu = sqrt(1 - u_a);  s = sqrt((1 - mu)*(1 + mu));  psi = (u_b*2)*pi;  sc = s*cos psi;  ss = s*sin psi   (polar)
//                e1, e2 = the frame about nrm (frame);  dir_k = (sc*e1_k + ss*e2_k) + mu*nrm_k                         (turned)
//   reflected:   v_k = c*dir_k;  dv_k = v_k - v_old_k;  dr_k = w*dir_k;  r_k = center_k + (x_k + dr_k)
//
// A phase function (PhaseFunctionStep): the photons the scatter step of this pass has hit (dv != 0) get a direction drawn about
// the direction they had BEFORE the scatter -- uniform on the sphere, Henyey-Greenstein or Rayleigh.  It joined this unit rather
// than a new one: the unit already includes pcl_device.h for the draws and holds the frame that turns (mu, psi) about an axis into
// a direction ("Adding a unit on the public ABI").
//
//   k_phase_redirect<T>    one grid-stride sweep: per slot the three dv rows (24 B in fp64), widened to double; lanes with a
//                          non-zero dv load v, and those whose old velocity o = v - dv has a length that can be worked with are
//                          counted (one ballot + popcount per wave, one LDS cell) and go on: they load their id, draw, and write
//                          v and dv.  r, dr and E are never looked at.
//
// Operation order (what light._phase_redirect restates with numpy):
//   scattered iff a photon and (dv0 != 0 or dv1 != 0 or dv2 != 0);  o_k = v_k - dv_k;  oo = o.o;  go on iff 0 < oo < inf
//   on = sqrt(oo);  w_k = o_k / on;  block A = counter (id_lo, id_hi, pass, 10): u_a, u_b
//   mu by the law (law_mu; include/physicl_hip.h writes the lines out): isotropic 1 - 2*u_a;  hg by the closed inverse for |g| >= 1/2
//   and by the same inverse written as a polynomial in g below it (good to 8 ulp(1) down to the smallest g), g == 0 the isotropic line;  rayleigh
//   3/4 uniform + 1/4 (3/2 mu^2): one lane in four takes the largest of three uniforms, block B = counter (id_lo, id_hi, pass, 11)
//   sc, ss = polar(mu, u_b);  e1, e2 = frame(w);  dir_k = (sc*e1_k + ss*e2_k) + mu*w_k;  v_k = c*dir_k;  dv_k = v_k - o_k
//
// An absorbing medium (AbsorptionStep): of the photons the scatter step of this pass has hit (dv != 0), those whose draw falls
// above the single-scattering albedo omega0 of the layer they stand in are absorbed: left in the store at rest where they are.
// It joined this unit as the phase function did: the unit holds the sweeps that rewrite photons and has the Philox block.
//
//   k_absorb_scattered<T>  one grid-stride sweep: per slot the three dv rows (24 B in fp64), widened to double; lanes with a
//                          non-zero dv are counted (one ballot + popcount per wave) and, with layers, load r and look q up in
//                          the squared edges (LDS, a binary search, no square root); lanes whose layer has omega0 < 1 load their
//                          id and draw; absorbed lanes are counted (a second ballot), write zeros to v and dv, add to their
//                          layer's cell and -- with energy bins -- load E and add to their layer's histogram.  Tallies are
//                          workgroup-private uint32 cells in LDS, flushed with 64-bit atomics.  dr and E are never written.
//
// Operation order (what light._absorb_scattered restates with numpy):
//   interacted iff a photon and (dv0 != 0 or dv1 != 0 or dv2 != 0);  no layers: b = 0;  layers: d = r - center;  q = d.d;
//   inside iff e2_0 <= q <= e2_L (NaN: false);  b = the bin of q in e2 = e*e: [e2_b, e2_(b+1)), the last one closed
//   inside and omega0_b < 1:  u = u53(w0, w1) of counter (id_lo, id_hi, pass, 12);  absorbed iff not (u < omega0_b)
//   absorbed:  v_k = 0;  dv_k = 0       (NOT the ground's dv = -v_old: a later sweep of this pass must see "did not scatter")
//
// Phase functions by layer (LayeredPhaseStep): the phase function's sweep with the absorber's layer search in front of the draw.
// Each radial layer mixes up to eight laws -- isotropic, Henyey-Greenstein, Rayleigh, or a tabulated piecewise-constant density --
// and a photon scattered inside a layer draws its law from the layer's weights, then its angle from the law.
//
//   k_phase_layered<T>     k_phase_redirect's sweep of the three dv rows; a scattered lane loads v and, with layers, r, and looks q
//                          up in the squared edges.  Lanes inside a layer choose a law (one more Philox block, counter word 13, only
//                          where the layer's row of weights is not one-hot), draw mu by that law -- a table by a binary search of
//                          its cumulative values and one multiply-add -- and turn about the old direction as k_phase_redirect does.
//                          All tables (cumulative weights, squared edges, g, and mu, F and the slopes of the tabulated laws) sit in
//                          dynamic LDS in front of the workgroup-private uint32 cells [scattered, re-directed | by layer | by law].
//
// Operation order (what light._layered_phase_redirect restates with numpy):
//   scattered iff a photon, dv != 0 and 0 < oo < inf (o, oo as above);  b: the absorber's layer of q (no layers: 0);  outside: counted
//   as scattered, not written;  inside:  law j = the first with u_s < C[b][j], u_s = u53(w0, w1) of counter (id_lo, id_hi, pass, 13)
//   isotropic, hg, rayleigh: the lines above, with the blocks 10 and 11;  table: k = the bin of u_a in F;
//   mu = min(max(mu_k + (u_a - F_k)*s_k, mu_k), mu_(k+1)),  s_k = (mu_(k+1) - mu_k) / (F_(k+1) - F_k) made on the host;  then as above
//
// A continuous source (RecycleStep): the photons the ground or the medium has left at rest, and those beyond the top of the
// atmosphere, are given back to a photon source: their slots are re-emitted, ids and kinds stay, the population is constant.
//
//   k_recycle_spent<T>     one grid-stride sweep: per slot the three v rows (only with at_rest; a lane whose v0 is not zero is
//                          decided and loads no more of them) and, for lanes that are not at rest, the three r rows (only with a
//                          top); two ballots + popcounts per wave for the two counters.  Only spent lanes go on: they load their
//                          id, draw the source's direction and position -- k_apply_source's emission (pcl_source.hip) with counter
//                          words of their own: the helpers are shared, source_mu and source_rho written out in both -- and write
//                          r, v, dr = 0 and dv = 0; with a spectrum they look a third draw up in the cumulative table (dynamic
//                          LDS, at most 16 KiB, in front of the two cells) and write E.
//
// Operation order (what light._recycle_spent restates with numpy):
//   rest = at_rest and v0 == 0 and v1 == 0 and v2 == 0;  d = r - center;  q = d.d;  gone = a top, not rest and q > top*top
//   spent iff a photon and (rest or gone);  direction: counter (id_lo, id_hi, pass, 14), position: (id_lo, id_hi, pass, 15), by the
//   arithmetic of pcl_store_apply_source;  dr = dv = 0;  E = grid[x], the first x with cdf[x] >= u53(w0, w1) of (id_lo, id_hi, pass, 16)
//
// Absorption along the path (PathAbsorptionStep): a gas that absorbs without scattering.  Every moving photon is exposed once per
// pass; the chance that it is absorbed over the move it has made, p = 1 - exp(-k c dt), is made on the host per radial layer and
// energy band, and the kernel only compares a draw with it.
//
//   k_absorb_path<T>       one grid-stride sweep: per slot v0 (a lane at rest -- k_recycle_spent's test -- loads v1 and v2 as well and
//                          nothing more; a moving lane is decided by v0 alone); moving lanes load, with layers, r and look q up in
//                          the squared edges (the absorber's search) and, with bands, E and look it up in the energy edges; a lane
//                          with a layer and a band is exposed, and if its cell's p is not zero it loads its id and draws; absorbed
//                          lanes write zeros to v and dv and add to their cell.  Two ballots + popcounts per wave for the two
//                          counters.  The tables (p, squared edges, energy edges) sit in dynamic LDS in front of the
//                          workgroup-private uint32 cells [exposed, absorbed | by cell].  r, dr and E are never written.
//
// Operation order (what light._absorb_path restates with numpy):
//   moving iff not (v0 == 0 and v1 == 0 and v2 == 0), a photon;  b: the absorber's layer of q (no layers: 0);  e: the bin of E in the
//   energy edges, the last one closed (no bands: 0);  exposed iff both exist;  p = P[b][e];  p > 0: u = u53(w0, w1) of counter
//   (id_lo, id_hi, pass, 17);  absorbed iff u < p:  v_k = 0;  dv_k = 0
//
// Re-emission in place (ReemissionStep): what the ground or the medium has absorbed is radiated again from where it was absorbed --
// a ground that glows in the infrared, a gas layer that returns its band, fluorescence with a lifetime.  A law, a spectrum and a
// yield per pass belong to the radial layer a photon is parked in.
//
//   k_reemit_parked<T>     one grid-stride sweep: per slot v0 (k_absorb_path's test the other way round: a moving lane is decided
//                          by v0 alone and loads nothing more; a lane at rest loads v1 and v2); lanes at rest load, with layers or a
//                          lambertian layer, r and look q up in the squared edges; a parked lane whose layer's eta is not zero loads
//                          its id and draws; re-emitted lanes draw a direction -- about (1, 0, 0), or cosine-weighted about the local
//                          vertical d / sqrt(q) --, write v, dr = 0 and dv = 0 and, if their layer has a table, look a third draw up
//                          in it and write E.  Two ballots + popcounts per wave for the two counters.  The tables (eta, squared
//                          edges, every layer's cdf and grid, 34 KiB at the most) sit in dynamic LDS in front of the
//                          workgroup-private uint32 cells [parked, re-emitted | by layer].  r, ids and kinds are never written.
//
// Operation order (what light._reemit_parked restates with numpy):
//   parked iff v0 == 0 and v1 == 0 and v2 == 0, a photon, with a layer b (the absorber's layer of q; no layers: 0)
//   eta_b > 0: u = u53(w0, w1) of counter (id_lo, id_hi, pass, 18);  re-emitted iff u < eta_b (lambertian: and 0 < q < inf)
//   (u_a, u_b) of counter (id_lo, id_hi, pass, 19);  isotropic: w = (1, 0, 0), mu = 1 - 2*u_a;  lambertian: w_k = d_k / sqrt(q),
//   mu = sqrt(1 - u_a);  e1, e2 = frame(w);  sc, ss = polar(mu, u_b);  v_k = c*turned;  dr_k = 0;  dv_k = 0
//   a table:  E = grid_b[x], the first x with cdf_b[x] >= u53(w0, w1) of counter (id_lo, id_hi, pass, 20)
//
// A refracting sphere (RefractiveSurfaceStep): a dielectric interface -- an ocean, a drop, the top of an atmosphere.  The ground's
// geometry for both crossing directions; where the ground bounces or parks, this sweep refracts by Snell's law or reflects with
// Fresnel's probability.  Directions change, speeds do not.
//
//   k_refract_surface<T>   k_surface_reflect's sweep of r and dr (48 B a slot in fp64); q_now and q_prev against R*R decide who
//                          crosses, and which way.  Only crossing lanes go on: they work the hit point, the facing normal and the
//                          outcome out in fp64, load their id and draw only where Fresnel's F > 0, load v and write r, v, dr, dv.
//                          The lanes meet again behind that block: one ballot + popcount per wave and counter (six LDS cells,
//                          flushed with 64-bit atomics), skipped by a wave nobody of which crosses.
//
// Operation order (what light._refract_surface restates with numpy):
//   d, m, p, q_now, q_prev as the ground's;  inward iff q_now < R2 <= q_prev < inf;  outward iff q_prev < R2 <= q_now < inf;  a photon
//   a = m.m;  b = p.m;  cq = q_prev - R2;  sq = sqrt(max(b*b - a*cq, 0));  inward: t = cq / (sq - b)
//   outward: t = min(max(b > 0 ? (0 - cq) / (sq + b) : (sq - b) / a, 0), 1)
//   x_k = p_k + t*m_k;  nrm_k = x_k / sqrt(x.x);  sa = sqrt(a);  mh_k = m_k / sa;  w = (1 - t)*sa
//   inward: N = nrm, eta = n_outside / n_inside;  outward: N = -nrm, eta = n_inside / n_outside      (the ratios made on the host)
//   ci = max(0 - mh.N, 0);  k = 1 - (eta*eta)*(1 - ci*ci);  k < 0: total, dir_k = mh_k + (2*ci)*N_k
//   ct = sqrt(k) (eta == 1: ct = ci);  ec = eta*ci;  rs = (ec - ct) / (ec + ct);  ect = eta*ct;  rp = (ci - ect) / (ci + ect)
//   F = (rs*rs + rp*rp)*0.5;  fresnel and F > 0: u = u53(w0, w1) of counter (id_lo, id_hi, pass, 21), reflected iff u < F: dir as above
//   refracted: dir_k = eta*mh_k + (ec - ct)*N_k
//   v_k = c*dir_k;  dv_k = v_k - v_old_k;  dr_k = w*dir_k;  y_k = x_k + dr_k;  r_k = center_k + y_k
//   overshot iff y.y >= R2 where the outcome ends inside (in refracted, out reflected, out total), y.y < R2 where it ends outside
//
// A spectral ground (SpectralSurfaceStep): the ground with an albedo and a mirrored share that depend on the band the photon's energy
// falls in -- vegetation, snow, water, a ground that is black in the infrared.  The ground's geometry, parking and flight; the band is
// k_absorb_path's lookup of E.  A hit photon in no band is absorbed: the ground stays opaque.
//
//   k_ground_spectral<T>   k_surface_reflect's sweep of r and dr (48 B a slot in fp64).  Only hit lanes go on: they load their kind, E
//                          and id, look the band up, draw (word 9 iff albedo_b < 1, the word of its own iff 0 < specular_b < 1) and
//                          meet the others at four ballots + popcounts per wave (reflected, absorbed, mirrored, out of band); then
//                          they add to their band's cell (an LDS atomic per lane), load v and write r, v, dr, dv as the ground does.
//                          The tables (albedo, specular, energy edges: 24 KiB at 1024 bands) sit in dynamic LDS in front of the
//                          workgroup-private uint32 cells [reflected, absorbed, mirrored, out of band | reflected by band |
//                          absorbed by band].  E, ids and kinds are never written.
//
// Operation order (what light._spectral_bounce restates with numpy):
//   hit: the ground's test;  e: the bin of (double)E in the energy edges, the last one closed (NaN and outside: no band)
//   no band: absorbed, out of band.  albedo_e < 1: u = u53(w0, w1) of counter (id_lo, id_hi, pass, 9); reflected iff u < albedo_e
//   reflected and 0 < specular_e < 1: u = u53(w0, w1) of counter (id_lo, id_hi, pass, 22); mirrored iff u < specular_e
//   (specular_e == 1: mirrored, == 0: not);  absorbed: the ground's park;  mirrored: the ground's specular line;  otherwise the
//   ground's lambertian lines with counter (id_lo, id_hi, pass, 8);  reflected: the ground's flight of the rest of the move
//
// Scattering by layer and band (LayeredScatterStep): who scatters, decided per radial layer and energy band -- a cloud's optical
// depth, an aerosol spectrum, a drop in vacuum.  k_absorb_path's exposure and draw against a probability made on the host; where that
// sweep parks, this one turns the photon into a direction uniform on the sphere (k_reemit_parked's isotropic lines) and leaves the
// scatter step's mark, dv = v' - v_old, for the phase and absorption sweeps behind it.
//
//   k_scatter_layered<T>   one grid-stride sweep: per slot the kind (a mixed store only) and v0 (a lane at rest loads v1 and v2 as well
//                          and nothing more; a moving lane is decided by v0 alone); moving photons load, with layers, r and, with
//                          bands, E, and look both up (k_absorb_path's searches); an exposed lane whose cell's p is not zero loads its
//                          id and draws.  Two ballots + popcounts per wave for the two counters.  With ``first`` every photon lane
//                          that is not hit stores zeros to its three dv rows -- one branch for the three rows, the whole wave in a
//                          uniform store.  Hit lanes add to their cell, load what they have not loaded of v, draw a direction and write
//                          v and dv.  The tables (p, squared edges, energy edges) sit in dynamic LDS in front of the workgroup-private
//                          uint32 cells [exposed, scattered | by cell].  r, dr and E are never written.
//
// Operation order (what light._scatter_layered restates with numpy):
//   moving, b, e, exposed, p = P[b][e]: k_absorb_path's lines;  p > 0: u = u53(w0, w1) of counter (id_lo, id_hi, pass, 23);
//   scattered iff u < p:  (u_a, u_b) of counter (id_lo, id_hi, pass, 24);  w = (1, 0, 0);  mu = 1 - 2*u_a;  e1, e2 = frame(w);
//   sc, ss = polar(mu, u_b);  v_k = c*turned;  dv_k = v_k - v_old_k;   first and a photon that is not scattered:  dv_k = 0
//
// Scattering on a grid of cells (GridScatterStep): who scatters, decided per cell of a one- to three-dimensional grid over x, y, z and
// the distance from a centre, and per energy band -- a cloud of finite width, a broken cloud field, a plume.  k_position_grid's cell,
// k_scatter_layered's exposure, draw, direction and mark.  The table may hold 2^20 probabilities: it does not always fit in LDS.
//
//   k_scatter_grid<T, lds>   one grid-stride sweep in k_scatter_layered's shape; a moving photon loads the r rows some axis needs and,
//                            with bands, E, and is looked up axis by axis in the edges (always in LDS).  lds = true: the
//                            probabilities and the workgroup's uint32 tallies by cell sit in LDS too (up to 4096 cells, the whole within
//                            64 KiB);  lds = false: p is a read-only load from the device table (8 MB at most, L2-resident over a
//                            sweep) and a hit adds to its cell in device memory with a 64-bit atomic.  In both forms the hit lanes of
//                            a wave that share one cell issue ONE add of their count, and one add for a whole run of such trips in
//                            the same cell (k_position_grid's ballot and compare): a bulk run starts with every photon in one cell.
//                            exposed and scattered are LDS counts fed from wave ballots in both forms.
//
// Operation order (what light._scatter_grid restates with numpy):
//   moving: k_scatter_layered's line;  cell: k_position_grid's lines, then the band as in k_absorb_path;  p = P[cell][e];
//   p > 0: u = u53(w0, w1) of counter (id_lo, id_hi, pass, 25);  scattered iff u < p:  (u_a, u_b) of counter (id_lo, id_hi, pass, 26);
//   the direction, v and dv: k_scatter_layered's lines;   first and a photon that is not scattered:  dv_k = 0
//
// Box walls (BoxBoundaryStep): the sides of the scene -- per axis a periodic, a mirror or an open wall, or none.  Deterministic: no
// draw, no id, no table.
//
//   k_box_walls<T>         one grid-stride sweep in k_absorb_path's shape: v decides a moving lane, which loads the r rows of the axes
//                          with a wall and is classified per axis (below / above / inside; a NaN or an infinity: skipped).  A lane
//                          outside on an open axis is parked (v = dv = 0); any other lane that is outside folds each such axis with one
//                          division and one floor.  The eight counts -- moving, multi, crossed[3][2] -- are wave ballots and popcounts
//                          into LDS above the continue of the lanes without work (the six of crossed and multi only in a wave that has
//                          such a lane), flushed once per workgroup.  A lane that crosses nothing writes nothing.
//
// Operation order (what light._box_walls restates with numpy):
//   moving: k_absorb_path's line;  below = x < lo;  above = x >= hi (periodic), x > hi (mirror, open);  open: park, first open axis counted;
//   s = x - lo;  n = floor(s / L);  f = min(max(s - n*L, 0), L);  periodic: y = lo + f, not (y < hi): y = lo;
//   mirror: h = n*0.5;  odd = floor(h) != h;  y = min(max(odd ? hi - f : lo + f, lo), hi);  odd: v_a, dv_a, dr_a negated
//
// Phase functions by grid cell (GridPhaseStep): how a scattered photon is turned, decided by the cell of k_position_grid's grid it
// stands in -- cloud droplets' forward peak in the cloudy columns, Rayleigh in the clear air beside them.  k_phase_layered's rule with
// the grid's cell in place of the radial layer: a cell names a MIXTURE, one of up to 64 rows of cumulative weights over the laws.
//
//   k_phase_grid<T>        k_phase_layered's grid-stride sweep of the three dv rows; a scattered lane loads v and the r rows some axis
//                          needs and is looked up axis by axis in the edges (LDS; k_position_grid's lines).  A lane with a cell reads
//                          ONE byte of the mixture map -- device memory, at most 1 MiB, L2-resident over a sweep; 255: left alone --,
//                          a lane in no cell takes the call's ``outside`` row (-1: left alone).  Then k_phase_layered's law draw, cosine
//                          (law_mu of pcl_rules.h for the closed-form laws, the table written out) and turn.  The tables (cumulative
//                          weights, edges, g, and mu, F and the slopes of the tabulated laws) sit in dynamic LDS in front of the
//                          workgroup-private uint32 cells [scattered, re-directed | by mixture | by law]; the whole stays within 64 KiB
//                          (the header states the bound; the largest law tables and the largest edge tables together do not fit).
//
// Operation order (what light_grid._grid_phase_redirect restates with numpy):
//   scattered: k_phase_layered's line;  cell: k_position_grid's lines;  m = map[cell], or ``outside`` in no cell;  m = none: counted as
//   scattered, not written;  otherwise law j = the first with u_s < C[m][j] (counter word 13), mu by the law (words 10 and 11) and the
//   turn about o/|o|: k_phase_layered's lines
//
// Absorption on a grid of cells (GridAbsorptionStep): who is absorbed -- along the path, by a probability p per cell and band, and at an
// interaction, by a single-scattering albedo per cell and band -- and the tally of the absorbed per cell, the heating field.  Both kinds
// in one sweep: these sweeps are bound by the store's traffic, and the cell lookup is the expensive part.
//
//   k_absorb_grid<T, lds>  the grid scatter's sweep without its direction: a moving photon loads the r rows some axis needs and, with
//                          bands, E, and is looked up in the edges (always in LDS); with an albedo table an exposed lane loads the
//                          three dv rows.  Which tables a call gives is uniform over the launch.  lds = true: the tables given and the
//                          workgroup's uint32 tallies by cell sit in LDS too (up to 4096 cells, the whole within 64 KiB: 4096 cells
//                          with one table, not with two);  lds = false: read-only loads from the device tables and 64-bit atomics on
//                          the device tallies.  The four counts are wave ballots and popcounts into LDS at the head of the body; the
//                          absorbed lanes of a wave that share a cell issue ONE add, and one add for a run of such trips in one cell.
//
// Operation order (what light_grid._grid_absorb restates with numpy):
//   moving, cell, band: the grid scatter's lines;  c = cell * B' + e;  interacted = dv != 0 (only with an albedo table);
//   p[c] > 0: u = u53(w0, w1) of counter (id_lo, id_hi, pass, 27), absorbed iff u < p[c];  otherwise, interacted and omega0[c] < 1:
//   u of counter (id_lo, id_hi, pass, 28), absorbed iff not (u < omega0[c]);  absorbed: v_k = 0, dv_k = 0;  anybody else is not written
#include "pcl_sweep.h"

#include "pcl_device.h" // (after the HIP runtime and the ABI's header, which pcl_sweep.h brings)
#include "pcl_rules.h"  // (after both)

namespace {

using namespace pcl_sweep;
using namespace pcl_rules;

template <typename T>
struct surface_args {
    T *r[3], *v[3], *dr[3], *dv[3];
    const unsigned char *kind;   // NULL: every particle is a photon
    const int64_t *ids;          // NULL: the id of slot i is id_base + i
    unsigned long long *out;     // [2]: reflected, absorbed; device, zeroed by the entry point
    int64_t N, ts, id_base;      // particles, tile stride of the slab (elements), id of slot 0
    int tile_log;                // log2 of the tile length (pcl_store_layout: 2048 particles)
    int mode;
    double c[3], R2, albedo, speed;
    uint32_t k0, k1, pass;       // Philox key (seed_lo, seed_hi), the step's own pass counter
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_surface_reflect(surface_args<T> a) {
    __shared__ uint32_t s_cnt[2];                                       // reflected, absorbed
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = grid_stride(), n_round = whole_waves(a.N);   // (the ballots below need whole waves inside the loop)
    for (int64_t i = first_slot(); i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        double d[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0}, p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (in) {
                d[k] = __dsub_rn((double)a.r[k][ti], a.c[k]);           // fp32 widens exactly
                m[k] = (double)a.dr[k][ti];
            }
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = __dsub_rn(d[k], m[k]);
        const double q_now = dot3(d, d), q_prev = dot3(p, p);
        // the shell sweep's inward crossing, of photons, with a previous position that can be worked with (NaN: false)
        bool hit = in && q_now < a.R2 && q_prev >= a.R2 && q_prev < INFINITY;
        if (hit && a.kind) hit = a.kind[i] != 0;
        uint64_t id = 0;
        bool refl = hit;
        if (hit) {
            id = id_of(a.ids, a.id_base, i);
            if (a.albedo < 1.0) refl = first_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, 9u, a.k0, a.k1)) < a.albedo;
        }
        const uint32_t n_hit = (uint32_t)__popcll(__ballot(hit)), n_refl = (uint32_t)__popcll(__ballot(refl));
        if (lane == 0 && n_refl) atomicAdd(&s_cnt[0], n_refl);
        if (lane == 0 && n_hit - n_refl) atomicAdd(&s_cnt[1], n_hit - n_refl);
        if (!hit) continue;     // lanes that are not hit wait at the loop's head: no ballot below this line
        const double aq = dot3(m, m), b = dot3(p, m), cq = __dsub_rn(q_prev, a.R2);
        const double disc = fmax(__dsub_rn(__dmul_rn(b, b), __dmul_rn(aq, cq)), 0.0);
        const double t = __ddiv_rn(cq, __dsub_rn(__dsqrt_rn(disc), b));
        double x[3], nrm[3], vo[3], dir[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            x[k] = __dadd_rn(p[k], __dmul_rn(t, m[k]));
            vo[k] = (double)a.v[k][ti];
        }
        if (!refl) {            // absorbed: parked on the sphere, at rest
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                a.r[k][ti] = (T)__dadd_rn(a.c[k], x[k]);
                a.v[k][ti] = (T)0.0;
                a.dr[k][ti] = (T)__dsub_rn(x[k], p[k]);
                a.dv[k][ti] = (T)__dsub_rn(0.0, vo[k]);
            }
            continue;
        }
        const double xn = __dsqrt_rn(dot3(x, x)), sa = __dsqrt_rn(aq);
#pragma unroll
        for (int k = 0; k < 3; ++k) nrm[k] = __ddiv_rn(x[k], xn);
        if (a.mode == PCL_SURFACE_SPECULAR) {
            double mh[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) mh[k] = __ddiv_rn(m[k], sa);
            const double dn2 = __dmul_rn(2.0, dot3(mh, nrm));
#pragma unroll
            for (int k = 0; k < 3; ++k) dir[k] = __dsub_rn(mh[k], __dmul_rn(dn2, nrm[k]));
        } else {
            double u_a, u_b, sc, ss, e1[3], e2[3];
            pair_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, 8u, a.k0, a.k1), &u_a, &u_b);
            const double mu = __dsqrt_rn(__dsub_rn(1.0, u_a));                                       // cosine-weighted hemisphere
            polar(mu, u_b, &sc, &ss);
            frame(nrm, e1, e2);
#pragma unroll
            for (int k = 0; k < 3; ++k) dir[k] = turned(sc, ss, mu, e1[k], e2[k], nrm[k]);
        }
        const double w = __dmul_rn(__dsub_rn(1.0, t), sa);              // the rest of the move, flown along the new direction
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double vk = __dmul_rn(a.speed, dir[k]), drk = __dmul_rn(w, dir[k]);
            a.r[k][ti] = (T)__dadd_rn(a.c[k], __dadd_rn(x[k], drk));
            a.v[k][ti] = (T)vk;
            a.dr[k][ti] = (T)drk;
            a.dv[k][ti] = (T)__dsub_rn(vk, vo[k]);
        }
    }
    __syncthreads();
    flush_cells(s_cnt, a.out, 2);
}

template <typename T>
struct phase_args {
    T *v[3], *dv[3];
    const unsigned char *kind;   // NULL: every particle is a photon
    const int64_t *ids;          // NULL: the id of slot i is id_base + i
    unsigned long long *out;     // [1]: re-directed; device, zeroed by the entry point
    int64_t N, ts, id_base;      // particles, tile stride of the slab (elements), id of slot 0
    int tile_log;                // log2 of the tile length
    int phase;
    double g, speed;
    uint32_t k0, k1, pass;       // Philox key (seed_lo, seed_hi), the step's own pass counter
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_phase_redirect(phase_args<T> a) {
    __shared__ uint32_t s_cnt[1];                                       // re-directed
    if (threadIdx.x == 0) s_cnt[0] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = grid_stride(), n_round = whole_waves(a.N);   // (the ballots below need whole waves inside the loop)
    for (int64_t i = first_slot(); i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        double d[3] = {0.0, 0.0, 0.0}, o[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (in) d[k] = (double)a.dv[k][ti];                         // fp32 widens exactly
        // scattered, written out (a helper changes the kernel): the scatter step left dv = v' - v_old on a hit, 0 on a miss (NaN != 0)
        bool go = in && (d[0] != 0.0 || d[1] != 0.0 || d[2] != 0.0);
        if (go && a.kind) go = a.kind[i] != 0;
        if (go) {
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = __dsub_rn((double)a.v[k][ti], d[k]);      // the velocity before the scatter
        }
        const double oo = dot3(o, o);
        go = go && oo > 0.0 && oo < INFINITY;                            // an old direction that can be worked with (NaN: false)
        const uint32_t n_go = (uint32_t)__popcll(__ballot(go));
        if (lane == 0 && n_go) atomicAdd(&s_cnt[0], n_go);
        if (!go) continue;      // lanes that are left alone wait at the loop's head: no ballot below this line
        const uint64_t id = id_of(a.ids, a.id_base, i);
        const double on = __dsqrt_rn(oo);
        double w[3], sc, ss, e1[3], e2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = __ddiv_rn(o[k], on);
        double u_a, u_b;
        pair_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, 10u, a.k0, a.k1), &u_a, &u_b);
        double mu = __dsub_rn(1.0, __dmul_rn(2.0, u_a));                                             // uniform on the sphere
        if (a.phase == PCL_PHASE_HG && a.g != 0.0) {
            const double gg = __dmul_rn(a.g, a.g);
            if (fabs(a.g) < 0.5) {                                      // the inverse as a polynomial in g: no difference of ones
                const double s = mu, gs = __dmul_rn(a.g, s), d = __dsub_rn(1.0, gs), s2 = __dmul_rn(s, s);
                const double p = __dadd_rn(__dsub_rn(__dmul_rn(0.5, __dadd_rn(s2, 3.0)), gs), __dmul_rn(gg, __dmul_rn(0.5, __dsub_rn(s2, 1.0))));
                mu = __ddiv_rn(__dsub_rn(__dmul_rn(a.g, p), s), __dmul_rn(d, d));
            } else {                                                    // the closed inverse
                const double g2 = __dmul_rn(2.0, a.g);
                const double q = __ddiv_rn(__dsub_rn(1.0, gg), __dadd_rn(__dsub_rn(1.0, a.g), __dmul_rn(g2, u_a)));
                mu = __ddiv_rn(__dsub_rn(__dadd_rn(1.0, gg), __dmul_rn(q, q)), g2);
            }
            mu = fmin(fmax(mu, -1.0), 1.0);
        } else if (a.phase == PCL_PHASE_RAYLEIGH) {
            const double s4 = __dmul_rn(u_a, 4.0), j = floor(s4);
            const double gq = __dsub_rn(__dmul_rn(2.0, __dsub_rn(s4, j)), 1.0);
            mu = gq;
            if (j == 3.0) {                                             // one lane in four: the 3/2 mu^2 part
                const pcl_u32x4 wb = pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, 11u, a.k0, a.k1);   // (pair_u53 changes the kernel)
                mu = copysign(fmax(fmax(fabs(gq), pcl_u53(wb.x, wb.y)), pcl_u53(wb.z, wb.w)), gq);
            }
        }
        polar(mu, u_b, &sc, &ss);
        frame(w, e1, e2);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double vk = __dmul_rn(a.speed, turned(sc, ss, mu, e1[k], e2[k], w[k]));
            a.v[k][ti] = (T)vk;
            a.dv[k][ti] = (T)__dsub_rn(vk, o[k]);
        }
    }
    __syncthreads();
    flush_cells(s_cnt, a.out, 1);
}

template <typename T>
struct absorb_args {
    const T *r[3];
    T *v[3], *dv[3];
    const T *E;                  // NULL without energy bins
    const unsigned char *kind;   // NULL: every particle is a photon
    const int64_t *ids;          // NULL: the id of slot i is id_base + i
    const double *tables;        // omega0 (L') | e*e of the layer edges (L + 1, if L) | E edges (n_E + 1, if any), device
    unsigned long long *out;     // interacted, absorbed | absorbed by layer [L'] | E_hist [L'][n_E]; device, zeroed by the entry point
    int64_t N, ts, id_base;      // particles, tile stride of the slab (elements), id of slot 0
    int tile_log;                // log2 of the tile length
    int n_layers, n_E;           // L (0: one omega0 everywhere, L' = 1), energy bins
    double c[3];
    uint32_t k0, k1, pass;       // Philox key (seed_lo, seed_hi), the step's own pass counter
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_absorb_scattered(absorb_args<T> a) {
    extern __shared__ double s_mem[];                                  // tables | interacted, absorbed | by layer | E histogram
    const int L = a.n_layers, Lp = L > 0 ? L : 1, nE = a.n_E;
    const int n_tab = Lp + (L ? L + 1 : 0) + (nE ? nE + 1 : 0);
    const int n_cells = 2 + Lp * (1 + nE);
    const double *s_om = s_mem;
    const double *s_e2 = s_om + Lp;
    const double *s_E = s_e2 + (L ? L + 1 : 0);
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_mem + n_tab);
    uint32_t *s_lay = s_cnt + 2;
    uint32_t *s_Eh = s_lay + Lp;
    for (int k = threadIdx.x; k < n_tab; k += kBlock) s_mem[k] = a.tables[k];
    for (int k = threadIdx.x; k < n_cells; k += kBlock) s_cnt[k] = 0;  // (the layers and the histograms follow the two counts)
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = grid_stride(), n_round = whole_waves(a.N);   // (the ballots below need whole waves inside the loop)
    for (int64_t i = first_slot(); i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        double d[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (in) d[k] = (double)a.dv[k][ti];                         // fp32 widens exactly
        // interacted in this pass: scattered, written out (a helper changes the kernel; NaN != 0 is true)
        bool go = in && (d[0] != 0.0 || d[1] != 0.0 || d[2] != 0.0);
        if (go && a.kind) go = a.kind[i] != 0;
        int b = go && L == 0 ? 0 : -1;                                  // the layer; -1: outside every layer, never absorbed
        if (go && L > 0) {
            double x[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = __dsub_rn((double)a.r[k][ti], a.c[k]);   // fp32 widens exactly
            const double q = dot3(x, x);
            if (q >= s_e2[0] && q <= s_e2[L]) b = bin_of(s_e2, L, q);   // (dist2, closed_bin: written out) NaN: in no layer
        }
        bool gone = false;
        if (b >= 0) {
            const double om = s_om[b];
            if (om < 1.0) {                                             // a conservative layer draws nothing
                const uint64_t id = id_of(a.ids, a.id_base, i);
                gone = !(first_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, 12u, a.k0, a.k1)) < om);      // the sense of the ground's albedo draw
            }
        }
        const uint32_t n_go = (uint32_t)__popcll(__ballot(go)), n_gone = (uint32_t)__popcll(__ballot(gone));
        if (lane == 0 && n_go) atomicAdd(&s_cnt[0], n_go);
        if (lane == 0 && n_gone) atomicAdd(&s_cnt[1], n_gone);
        if (!gone) continue;    // lanes that are left alone wait at the loop's head: no ballot below this line
#pragma unroll
        for (int k = 0; k < 3; ++k) {                                   // park, written out: at rest where it is; "did not scatter"
            a.v[k][ti] = (T)0.0;
            a.dv[k][ti] = (T)0.0;
        }
        atomicAdd(&s_lay[b], 1u);
        if (nE) {
            const double e = (double)a.E[ti];
            if (e >= s_E[0] && e <= s_E[nE]) atomicAdd(&s_Eh[b * nE + bin_of(s_E, nE, e)], 1u);   // NaN and under/overflow: in no bin
        }
    }
    __syncthreads();
    // pcl_sweep::flush_cells, written out: its other two callers in this unit hand it a literal 1 or 2 cells, which the compiler
    // folds into the helper before it inlines it; a third caller with a count that is not a literal takes that away and changes
    // the epilogue of k_phase_redirect (tools/compare_unit_asm.py shows it).  In place, the two kernels stay the code they were.
    for (int k = threadIdx.x; k < n_cells; k += kBlock)
        if (s_cnt[k]) atomicAdd(&a.out[k], (unsigned long long)s_cnt[k]);
}

// The counter word of the draw that chooses a law (the header lists who uses which word: 13 is this kernel's and k_phase_grid's).
constexpr uint32_t kLawWord = 13;

template <typename T>
struct lphase_args {
    const T *r[3];
    T *v[3], *dv[3];
    const unsigned char *kind;   // NULL: every particle is a photon
    const int64_t *ids;          // NULL: the id of slot i is id_base + i
    const double *tables;        // C (L' x M) | e*e of the layer edges (L + 1, if L) | g (M) | mu, F, s (n_nodes each) | the laws' ints
    unsigned long long *out;     // scattered, re-directed | by layer [L'] | by law [M]; device, zeroed by the entry point
    int64_t N, ts, id_base;      // particles, tile stride of the slab (elements), id of slot 0
    int tile_log;                // log2 of the tile length
    int n_layers, n_laws;        // L (0: one row of C everywhere, L' = 1), M
    int n_nodes;                 // the nodes of all tables, K + 1 each (0 without a table)
    double c[3], speed;
    uint32_t k0, k1, pass;       // Philox key (seed_lo, seed_hi), the step's own pass counter
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_phase_layered(lphase_args<T> a) {
    extern __shared__ double s_mem[];                                  // tables | scattered, re-directed | by layer | by law
    const int L = a.n_layers, Lp = L > 0 ? L : 1, M = a.n_laws, Tn = a.n_nodes;
    const int n_dbl = Lp * M + (L ? L + 1 : 0) + M + 3 * Tn;
    const int n_tab = n_dbl + (3 * M + 1) / 2;                         // three ints per law, packed behind the doubles
    const int n_cells = 2 + Lp + M;
    const double *s_C = s_mem;
    const double *s_e2 = s_C + Lp * M;
    const double *s_g = s_e2 + (L ? L + 1 : 0);
    const double *s_mu = s_g + M;
    const double *s_F = s_mu + Tn;
    const double *s_s = s_F + Tn;
    const int *s_kind = reinterpret_cast<const int *>(s_mem + n_dbl);  // PCL_PHASE_* of law j
    const int *s_off = s_kind + M;                                     // a table's first node in mu, F and s
    const int *s_K = s_off + M;                                        // a table's bins
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_mem + n_tab);
    uint32_t *s_lay = s_cnt + 2;
    uint32_t *s_law = s_lay + Lp;
    for (int k = threadIdx.x; k < n_tab; k += kBlock) s_mem[k] = a.tables[k];
    for (int k = threadIdx.x; k < n_cells; k += kBlock) s_cnt[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = grid_stride(), n_round = whole_waves(a.N);   // (the ballots below need whole waves inside the loop)
    for (int64_t i = first_slot(); i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        double d[3] = {0.0, 0.0, 0.0}, o[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (in) d[k] = (double)a.dv[k][ti];                         // fp32 widens exactly
        // scattered in this pass: scattered and workable, written out (a helper changes the kernel)
        bool go = in && (d[0] != 0.0 || d[1] != 0.0 || d[2] != 0.0);
        if (go && a.kind) go = a.kind[i] != 0;
        if (go) {
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = __dsub_rn((double)a.v[k][ti], d[k]);      // the velocity before the scatter
        }
        const double oo = dot3(o, o);
        go = go && oo > 0.0 && oo < INFINITY;
        int b = go && L == 0 ? 0 : -1;                                  // the layer; -1: outside every layer, left as the scatter step left it
        if (go && L > 0) {
            double x[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = __dsub_rn((double)a.r[k][ti], a.c[k]);   // fp32 widens exactly
            const double q = dot3(x, x);
            if (q >= s_e2[0] && q <= s_e2[L]) b = bin_of(s_e2, L, q);   // (dist2, closed_bin: written out) NaN: in no layer
        }
        const bool turn = b >= 0;
        const uint32_t n_go = (uint32_t)__popcll(__ballot(go)), n_turn = (uint32_t)__popcll(__ballot(turn));
        if (lane == 0 && n_go) atomicAdd(&s_cnt[0], n_go);
        if (lane == 0 && n_turn) {
            atomicAdd(&s_cnt[1], n_turn);
            if (Lp == 1) atomicAdd(&s_lay[0], n_turn);                  // one layer, one law: the wave's count, not a lane's
            if (M == 1) atomicAdd(&s_law[0], n_turn);
        }
        if (!turn) continue;    // lanes that are left alone wait at the loop's head: no ballot below this line
        const uint64_t id = id_of(a.ids, a.id_base, i);
        int j = 0;
        if (M > 1) {
            const double *row = s_C + b * M;                            // cumulative, ends in 1: the first j with u_s < row[j]
            while (j < M - 1 && !(row[j] > 0.0)) ++j;                   // (u_s >= 0: a law without weight is never the first)
            if (row[j] < 1.0) {                                         // a one-hot row draws nothing
                const double u_s = first_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kLawWord, a.k0, a.k1));
                while (j < M - 1 && !(u_s < row[j])) ++j;
            }
            atomicAdd(&s_law[j], 1u);
        }
        if (Lp > 1) atomicAdd(&s_lay[b], 1u);
        const double on = __dsqrt_rn(oo);
        double w[3], sc, ss, e1[3], e2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = __ddiv_rn(o[k], on);
        double u_a, u_b;
        pair_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, 10u, a.k0, a.k1), &u_a, &u_b);
        const int law = s_kind[j];
        const double g = s_g[j];
        double mu = __dsub_rn(1.0, __dmul_rn(2.0, u_a));                                             // uniform on the sphere
        if (law == PCL_PHASE_HG && g != 0.0) {                                 // law_mu, written out in both phase kernels
            const double gg = __dmul_rn(g, g);
            if (fabs(g) < 0.5) {                                        // the inverse as a polynomial in g: no difference of ones
                const double s = mu, gs = __dmul_rn(g, s), d = __dsub_rn(1.0, gs), s2 = __dmul_rn(s, s);
                const double p = __dadd_rn(__dsub_rn(__dmul_rn(0.5, __dadd_rn(s2, 3.0)), gs), __dmul_rn(gg, __dmul_rn(0.5, __dsub_rn(s2, 1.0))));
                mu = __ddiv_rn(__dsub_rn(__dmul_rn(g, p), s), __dmul_rn(d, d));
            } else {                                                    // the closed inverse
                const double g2 = __dmul_rn(2.0, g);
                const double q = __ddiv_rn(__dsub_rn(1.0, gg), __dadd_rn(__dsub_rn(1.0, g), __dmul_rn(g2, u_a)));
                mu = __ddiv_rn(__dsub_rn(__dadd_rn(1.0, gg), __dmul_rn(q, q)), g2);
            }
            mu = fmin(fmax(mu, -1.0), 1.0);
        } else if (law == PCL_PHASE_RAYLEIGH) {
            const double s4 = __dmul_rn(u_a, 4.0), jq = floor(s4);
            const double gq = __dsub_rn(__dmul_rn(2.0, __dsub_rn(s4, jq)), 1.0);
            mu = gq;
            if (jq == 3.0) {                                            // one lane in four: the 3/2 mu^2 part
                const pcl_u32x4 wb = pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, 11u, a.k0, a.k1);   // (pair_u53 changes the kernel)
                mu = copysign(fmax(fmax(fabs(gq), pcl_u53(wb.x, wb.y)), pcl_u53(wb.z, wb.w)), gq);
            }
        } else if (law == PCL_PHASE_TABLE) {                            // the inverse of a piecewise linear F: 0 <= u_a < 1 is inside
            const int off = s_off[j];
            const int kb = off + bin_of(s_F + off, s_K[j], u_a);
            const double lo = s_mu[kb], hi = s_mu[kb + 1];
            mu = fmin(fmax(__dadd_rn(lo, __dmul_rn(__dsub_rn(u_a, s_F[kb]), s_s[kb])), lo), hi);
        }
        polar(mu, u_b, &sc, &ss);
        frame(w, e1, e2);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double vk = __dmul_rn(a.speed, turned(sc, ss, mu, e1[k], e2[k], w[k]));
            a.v[k][ti] = (T)vk;
            a.dv[k][ti] = (T)__dsub_rn(vk, o[k]);
        }
    }
    __syncthreads();
    // pcl_sweep::flush_cells, written out, for the reason given in k_absorb_scattered: the count is not a literal
    for (int k = threadIdx.x; k < n_cells; k += kBlock)
        if (s_cnt[k]) atomicAdd(&a.out[k], (unsigned long long)s_cnt[k]);
}

// The counter words of a re-emission (the header lists who uses which word: 14, 15 and 16 are this kernel's alone).
constexpr uint32_t kRecycleDirWord = 14, kRecyclePosWord = 15, kRecycleEnergyWord = 16;

template <typename T>
struct recycle_args {
    T *r[3], *v[3], *dr[3], *dv[3];
    T *E;                        // NULL without a spectrum: a recycled photon keeps its energy
    const unsigned char *kind;   // NULL: every particle is a photon
    const int64_t *ids;          // NULL: the id of slot i is id_base + i
    const double *tables;        // cdf (n_E) | grid (n_E), device; unused without a spectrum
    unsigned long long *out;     // [2]: at rest, escaped; device, zeroed by the entry point
    int64_t N, ts, id_base;      // particles, tile stride of the slab (elements), id of slot 0
    int tile_log;                // log2 of the tile length
    int at_rest, has_top, n_E;   // the two criteria, the bins of the spectrum (0: none)
    int angular, spatial;        // PCL_SRC_*
    double c[3], top2;           // the centre, top*top (made on the host)
    double origin[3], e1[3], e2[3], d[3];
    double speed, cos_half_angle, radius;
    uint32_t k0, k1, pass;       // Philox key (seed_lo, seed_hi), the step's own pass counter
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_recycle_spent(recycle_args<T> a) {
    extern __shared__ double s_mem[];                                  // cdf | grid | at rest, escaped
    const int nE = a.n_E;
    const double *s_cdf = s_mem;
    const double *s_grid = s_mem + nE;
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_mem + 2 * nE);
    for (int k = threadIdx.x; k < 2 * nE; k += kBlock) s_mem[k] = a.tables[k];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = grid_stride(), n_round = whole_waves(a.N);   // (the ballots below need whole waves inside the loop)
    for (int64_t i = first_slot(); i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        bool rest = false, gone = false;
        if (in && a.at_rest)                                            // -0.0 == 0; a NaN is not at rest (fp32 widens exactly)
            rest = (double)a.v[0][ti] == 0.0 && (double)a.v[1][ti] == 0.0 && (double)a.v[2][ti] == 0.0;
        if (in && a.has_top && !rest) {
            double x[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = __dsub_rn((double)a.r[k][ti], a.c[k]);
            gone = dot3(x, x) > a.top2;                                 // on the sphere: not gone; NaN: not gone; inf: gone
        }
        if ((rest || gone) && a.kind && a.kind[i] == 0) rest = gone = false;             // plain Objects are never spent
        const uint32_t n_rest = (uint32_t)__popcll(__ballot(rest)), n_gone = (uint32_t)__popcll(__ballot(gone));
        if (lane == 0 && n_rest) atomicAdd(&s_cnt[0], n_rest);
        if (lane == 0 && n_gone) atomicAdd(&s_cnt[1], n_gone);
        if (!(rest || gone)) continue;   // lanes that are left alone wait at the loop's head: no ballot below this line
        const uint64_t id = id_of(a.ids, a.id_base, i);
        double vel[3], pos[3];
        if (a.angular == PCL_SRC_BEAM) {                                // a constant: no draw
#pragma unroll
            for (int k = 0; k < 3; ++k) vel[k] = __dmul_rn(a.speed, a.d[k]);
        } else {
            double u_a, u_b, sc, ss;
            pair_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kRecycleDirWord, a.k0, a.k1), &u_a, &u_b);
            double mu;      // source_mu, in place in both emitters (a helper changes the kernels): the cosine of the polar angle about d
            if (a.angular == PCL_SRC_ISOTROPIC)
                mu = __dsub_rn(1.0, __dmul_rn(2.0, u_a));                                         // uniform on the sphere
            else if (a.angular == PCL_SRC_CONE)
                mu = __dsub_rn(1.0, __dmul_rn(u_a, __dsub_rn(1.0, a.cos_half_angle)));            // uniform in solid angle
            else
                mu = __dsqrt_rn(__dsub_rn(1.0, u_a));                                             // cosine-weighted hemisphere
            polar(mu, u_b, &sc, &ss);
#pragma unroll
            for (int k = 0; k < 3; ++k) vel[k] = __dmul_rn(a.speed, turned(sc, ss, mu, a.e1[k], a.e2[k], a.d[k]));
        }
        if (a.spatial == PCL_SRC_POINT) {
#pragma unroll
            for (int k = 0; k < 3; ++k) pos[k] = a.origin[k];
        } else {
            double u_c, u_d, rc, rs;
            pair_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kRecyclePosWord, a.k0, a.k1), &u_c, &u_d);
            double rho;     // source_rho, in place in both emitters (a helper changes the kernels): the distance from the origin
            if (a.spatial == PCL_SRC_DISC)
                rho = __dmul_rn(a.radius, __dsqrt_rn(u_c));                                       // uniform over the disc
            else                                                                                  // 1 - u_c is in (0, 1]
                rho = __dmul_rn(a.radius, __dsqrt_rn(__dmul_rn(-2.0, log(__dsub_rn(1.0, u_c)))));
            azimuth(rho, u_d, &rc, &rs);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                pos[k] = __dadd_rn(a.origin[k], __dadd_rn(__dmul_rn(rc, a.e1[k]), __dmul_rn(rs, a.e2[k])));
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {                                   // a newborn has not moved and has not scattered
            a.r[k][ti] = (T)pos[k];
            a.v[k][ti] = (T)vel[k];
            a.dr[k][ti] = (T)0.0;
            a.dv[k][ti] = (T)0.0;
        }
        if (nE) {                                                       // the first x with cdf[x] >= u (cdf ends in 1 > u): compares only
            const double u = first_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kRecycleEnergyWord, a.k0, a.k1));
            int lo = 0, hi = nE - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_cdf[mid] >= u) hi = mid; else lo = mid + 1;
            }
            a.E[ti] = (T)s_grid[lo];
        }
    }
    __syncthreads();
    // pcl_sweep::flush_cells, written out, for the reason given in k_absorb_scattered: a further caller changes the older kernels
    for (int k = threadIdx.x; k < 2; k += kBlock)
        if (s_cnt[k]) atomicAdd(&a.out[k], (unsigned long long)s_cnt[k]);
}

// The counter word of the draw along the path (the header lists who uses which word: 17 is this kernel's alone).
constexpr uint32_t kPathAbsorbWord = 17;

template <typename T>
struct pabsorb_args {
    const T *r[3];               // read only with layers
    T *v[3], *dv[3];
    const T *E;                  // NULL without energy bands
    const unsigned char *kind;   // NULL: every particle is a photon
    const int64_t *ids;          // NULL: the id of slot i is id_base + i
    const double *tables;        // p (L' x B') | e*e of the layer edges (L + 1, if L) | E edges (B + 1, if B), device
    unsigned long long *out;     // exposed, absorbed | absorbed by cell [L' x B']; device, zeroed by the entry point
    int64_t N, ts, id_base;      // particles, tile stride of the slab (elements), id of slot 0
    int tile_log;                // log2 of the tile length
    int n_layers, n_E;           // L (0: one row of p everywhere, L' = 1), B (0: one column for every energy, B' = 1)
    double c[3];
    uint32_t k0, k1, pass;       // Philox key (seed_lo, seed_hi), the step's own pass counter
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_absorb_path(pabsorb_args<T> a) {
    extern __shared__ double s_mem[];                                  // p | e*e | E edges | exposed, absorbed | by cell
    const int L = a.n_layers, Lp = L > 0 ? L : 1, nE = a.n_E, Bp = nE > 0 ? nE : 1;
    const int n_tab = Lp * Bp + (L ? L + 1 : 0) + (nE ? nE + 1 : 0);
    const int n_cells = 2 + Lp * Bp;
    const double *s_p = s_mem;
    const double *s_e2 = s_p + Lp * Bp;
    const double *s_E = s_e2 + (L ? L + 1 : 0);
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_mem + n_tab);
    uint32_t *s_cell = s_cnt + 2;
    for (int k = threadIdx.x; k < n_tab; k += kBlock) s_mem[k] = a.tables[k];
    for (int k = threadIdx.x; k < n_cells; k += kBlock) s_cnt[k] = 0;  // (the cells follow the two counts)
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = grid_stride(), n_round = whole_waves(a.N);   // (the ballots below need whole waves inside the loop)
    for (int64_t i = first_slot(); i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        // moving: at_rest, written out (a helper changes the kernel) and negated -- -0.0 == 0, a NaN moves, v0 != 0 loads no more of v
        bool go = in && !((double)a.v[0][ti] == 0.0 && (double)a.v[1][ti] == 0.0 && (double)a.v[2][ti] == 0.0);
        if (go && a.kind) go = a.kind[i] != 0;                          // plain Objects are never touched
        int b = go && L == 0 ? 0 : -1;                                  // the layer; -1: in no layer
        if (go && L > 0) {
            double x[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = __dsub_rn((double)a.r[k][ti], a.c[k]);   // fp32 widens exactly
            const double q = dot3(x, x);
            if (q >= s_e2[0] && q <= s_e2[L]) b = bin_of(s_e2, L, q);   // (dist2, closed_bin: written out) NaN: in no layer
        }
        int cell = b >= 0 && nE == 0 ? b : -1;                          // b * B' + e; -1: not exposed
        if (b >= 0 && nE > 0) {
            const double e = (double)a.E[ti];
            if (e >= s_E[0] && e <= s_E[nE]) cell = b * nE + bin_of(s_E, nE, e);         // NaN and under/overflow: in no band
        }
        const bool exposed = cell >= 0;
        bool gone = false;
        if (exposed) {
            const double p = s_p[cell];
            if (p > 0.0) {                                              // a transparent cell draws nothing
                const uint64_t id = id_of(a.ids, a.id_base, i);
                gone = first_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kPathAbsorbWord, a.k0, a.k1)) < p;   // u < 1: p == 1 absorbs everybody
            }
        }
        const uint32_t n_exp = (uint32_t)__popcll(__ballot(exposed)), n_gone = (uint32_t)__popcll(__ballot(gone));
        if (lane == 0 && n_exp) atomicAdd(&s_cnt[0], n_exp);
        if (lane == 0 && n_gone) atomicAdd(&s_cnt[1], n_gone);
        if (!gone) continue;    // lanes that are left alone wait at the loop's head: no ballot below this line
#pragma unroll
        for (int k = 0; k < 3; ++k) {                                   // park, written out: at rest where it is; "did not scatter"
            a.v[k][ti] = (T)0.0;
            a.dv[k][ti] = (T)0.0;
        }
        atomicAdd(&s_cell[cell], 1u);
    }
    __syncthreads();
    // pcl_sweep::flush_cells, written out, for the reason given in k_absorb_scattered: the count is not a literal
    for (int k = threadIdx.x; k < n_cells; k += kBlock)
        if (s_cnt[k]) atomicAdd(&a.out[k], (unsigned long long)s_cnt[k]);
}

// The counter words of a re-emission in place: who is re-emitted, where to, with which energy (the header lists who uses which
// word: 18, 19 and 20 are this kernel's alone).
constexpr uint32_t kReemitDraw = 18, kReemitDir = 19, kReemitEnergy = 20;

template <typename T>
struct reemit_args {
    const T *r[3];               // read only with layers or a lambertian layer
    T *v[3], *dr[3], *dv[3];
    T *E;                        // NULL if no layer has a table: a re-emitted photon keeps its energy
    const unsigned char *kind;   // NULL: every particle is a photon
    const int64_t *ids;          // NULL: the id of slot i is id_base + i
    const double *tables;        // eta (L') | e*e of the layer edges (L + 1, if L) | cdf (n_bins) | grid (n_bins) | the layers' ints
    unsigned long long *out;     // parked, re-emitted | by layer [L']; device, zeroed by the entry point
    int64_t N, ts, id_base;      // particles, tile stride of the slab (elements), id of slot 0
    int tile_log;                // log2 of the tile length
    int n_layers, n_bins;        // L (0: one layer everywhere, L' = 1), the bins of all tables together
    int need_r;                  // layers, or a lambertian layer: somebody's position matters
    double c[3], speed;
    uint32_t k0, k1, pass;       // Philox key (seed_lo, seed_hi), the step's own pass counter
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_reemit_parked(reemit_args<T> a) {
    extern __shared__ double s_mem[];                                  // tables | parked, re-emitted | by layer
    const int L = a.n_layers, Lp = L > 0 ? L : 1, nB = a.n_bins;
    const int n_dbl = Lp + (L ? L + 1 : 0) + 2 * nB;
    const int n_tab = n_dbl + (2 * Lp + 2) / 2;                         // 2 L' + 1 ints, packed behind the doubles
    const int n_cells = 2 + Lp;
    const double *s_eta = s_mem;
    const double *s_e2 = s_eta + Lp;
    const double *s_cdf = s_e2 + (L ? L + 1 : 0);
    const double *s_grid = s_cdf + nB;
    const int *s_lam = reinterpret_cast<const int *>(s_mem + n_dbl);   // 1: layer b emits cosine-weighted about the local vertical
    const int *s_off = s_lam + Lp;                                     // layer b's table: [s_off[b], s_off[b + 1]) of cdf and grid
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_mem + n_tab);
    uint32_t *s_lay = s_cnt + 2;
    for (int k = threadIdx.x; k < n_tab; k += kBlock) s_mem[k] = a.tables[k];
    for (int k = threadIdx.x; k < n_cells; k += kBlock) s_cnt[k] = 0;  // (the layers follow the two counts)
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = grid_stride(), n_round = whole_waves(a.N);   // (the ballots below need whole waves inside the loop)
    for (int64_t i = first_slot(); i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        // at_rest, written out as in k_absorb_path: -0.0 == 0, a NaN moves, v0 != 0 loads no more of v (fp32 widens exactly)
        bool rest = in && (double)a.v[0][ti] == 0.0 && (double)a.v[1][ti] == 0.0 && (double)a.v[2][ti] == 0.0;
        if (rest && a.kind) rest = a.kind[i] != 0;                      // plain Objects are never re-emitted
        double d[3] = {0.0, 0.0, 0.0};
        if (rest && a.need_r) {
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = __dsub_rn((double)a.r[k][ti], a.c[k]);   // fp32 widens exactly
        }
        const double q = dot3(d, d);
        int b = rest && L == 0 ? 0 : -1;                                // the layer; -1: in no layer, left parked
        if (rest && L > 0 && q >= s_e2[0] && q <= s_e2[L]) b = bin_of(s_e2, L, q);      // (dist2, closed_bin: written out) NaN: in no layer
        const bool parked = b >= 0;
        bool go = false;
        uint64_t id = 0;
        if (parked) {
            const double eta = s_eta[b];
            if (eta > 0.0) {                                            // a layer that holds what it absorbed draws nothing
                id = id_of(a.ids, a.id_base, i);
                go = first_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kReemitDraw, a.k0, a.k1)) < eta;   // u < 1: eta == 1 re-emits everybody
                if (go && s_lam[b]) go = q > 0.0 && q < INFINITY;       // no vertical at the centre (or with a NaN): parked only
            }
        }
        const uint32_t n_parked = (uint32_t)__popcll(__ballot(parked)), n_go = (uint32_t)__popcll(__ballot(go));
        if (lane == 0 && n_parked) atomicAdd(&s_cnt[0], n_parked);
        if (lane == 0 && n_go) {
            atomicAdd(&s_cnt[1], n_go);
            if (Lp == 1) atomicAdd(&s_lay[0], n_go);                    // one layer: the wave's count, not a lane's
        }
        if (!go) continue;      // lanes that are left alone wait at the loop's head: no ballot below this line
        if (Lp > 1) atomicAdd(&s_lay[b], 1u);
        double u_a, u_b, sc, ss, w[3] = {1.0, 0.0, 0.0}, e1[3], e2[3];
        pair_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kReemitDir, a.k0, a.k1), &u_a, &u_b);
        double mu = __dsub_rn(1.0, __dmul_rn(2.0, u_a));                                             // uniform on the sphere
        if (s_lam[b]) {
            const double s = __dsqrt_rn(q);
#pragma unroll
            for (int k = 0; k < 3; ++k) w[k] = __ddiv_rn(d[k], s);      // the local vertical
            mu = __dsqrt_rn(__dsub_rn(1.0, u_a));                                                    // cosine-weighted hemisphere
        }
        polar(mu, u_b, &sc, &ss);
        frame(w, e1, e2);
#pragma unroll
        for (int k = 0; k < 3; ++k) {                                   // it has neither moved nor scattered
            a.v[k][ti] = (T)__dmul_rn(a.speed, turned(sc, ss, mu, e1[k], e2[k], w[k]));
            a.dr[k][ti] = (T)0.0;
            a.dv[k][ti] = (T)0.0;
        }
        int lo = s_off[b], hi = s_off[b + 1] - 1;
        if (hi >= lo) {                                                 // the first x with cdf[x] >= u (the table ends in 1 > u): compares only
            const double u = first_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kReemitEnergy, a.k0, a.k1));
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_cdf[mid] >= u) hi = mid; else lo = mid + 1;
            }
            a.E[ti] = (T)s_grid[lo];
        }
    }
    __syncthreads();
    // pcl_sweep::flush_cells, written out, for the reason given in k_absorb_scattered: the count is not a literal
    for (int k = threadIdx.x; k < n_cells; k += kBlock)
        if (s_cnt[k]) atomicAdd(&a.out[k], (unsigned long long)s_cnt[k]);
}

// The counter word of the Fresnel draw (the header lists who uses which word: 21 is this kernel's alone).
constexpr uint32_t kRefractDraw = 21;

template <typename T>
struct refract_args {
    T *r[3], *v[3], *dr[3], *dv[3];
    const unsigned char *kind;   // NULL: every particle is a photon
    const int64_t *ids;          // NULL: the id of slot i is id_base + i
    unsigned long long *out;     // [6]: in refracted, in reflected, out refracted, out reflected, out total, overshot; device, zeroed
    int64_t N, ts, id_base;      // particles, tile stride of the slab (elements), id of slot 0
    int tile_log;                // log2 of the tile length
    int fresnel;                 // 0: nothing is drawn, every crossing that is not total refracts
    double c[3], R2, speed;
    double eta_in, eta_out;      // n_outside / n_inside, n_inside / n_outside (made on the host)
    uint32_t k0, k1, pass;       // Philox key (seed_lo, seed_hi), the step's own pass counter
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_refract_surface(refract_args<T> a) {
    __shared__ uint32_t s_cnt[6];
    if (threadIdx.x < 6) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = grid_stride(), n_round = whole_waves(a.N);   // (the ballots below need whole waves inside the loop)
    for (int64_t i = first_slot(); i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        double d[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0}, p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (in) {
                d[k] = __dsub_rn((double)a.r[k][ti], a.c[k]);           // fp32 widens exactly
                m[k] = (double)a.dr[k][ti];
            }
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = __dsub_rn(d[k], m[k]);
        const double q_now = dot3(d, d), q_prev = dot3(p, p);
        // the ground's inward crossing, and the same the other way round (on the sphere is outside; NaN: false)
        const bool inward = in && q_now < a.R2 && q_prev >= a.R2 && q_prev < INFINITY;
        const bool outward = in && q_prev < a.R2 && q_now >= a.R2 && q_now < INFINITY;
        bool cross = inward || outward;
        if (cross && a.kind) cross = a.kind[i] != 0;
        int outcome = -1;       // the cell: 0 in refracted, 1 in reflected, 2 out refracted, 3 out reflected, 4 out total
        bool over = false;
        if (cross) {            // (no ballot inside: the lanes meet again behind this block)
            const double aq = dot3(m, m), b = dot3(p, m), cq = __dsub_rn(q_prev, a.R2);
            const double sq = __dsqrt_rn(fmax(__dsub_rn(__dmul_rn(b, b), __dmul_rn(aq, cq)), 0.0));
            double t;
            if (inward)                                                 // the ground's root
                t = __ddiv_rn(cq, __dsub_rn(sq, b));
            else                                                        // the other root, in the form that does not cancel
                t = fmin(fmax(b > 0.0 ? __ddiv_rn(__dsub_rn(0.0, cq), __dadd_rn(sq, b)) : __ddiv_rn(__dsub_rn(sq, b), aq), 0.0), 1.0);
            double x[3], nf[3], mh[3], dir[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = __dadd_rn(p[k], __dmul_rn(t, m[k]));
            const double xn = __dsqrt_rn(dot3(x, x)), sa = __dsqrt_rn(aq);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double nrm = __ddiv_rn(x[k], xn);
                nf[k] = inward ? nrm : -nrm;                            // the normal that faces the photon
                mh[k] = __ddiv_rn(m[k], sa);
            }
            const double w = __dmul_rn(__dsub_rn(1.0, t), sa);          // the rest of the move, flown along the new direction
            const double eta = inward ? a.eta_in : a.eta_out;
            const double ci = fmax(__dsub_rn(0.0, dot3(mh, nf)), 0.0);
            const double kk = __dsub_rn(1.0, __dmul_rn(__dmul_rn(eta, eta), __dsub_rn(1.0, __dmul_rn(ci, ci))));
            bool refl = kk < 0.0;                                       // total internal reflection: no draw
            double ec = 0.0, ct = 0.0;
            if (refl) {
                outcome = inward ? 1 : 4;                               // (inward, with n_outside > n_inside: counted as reflected)
            } else {
                ct = eta == 1.0 ? ci : __dsqrt_rn(kk);                  // no interface: the photon passes, whatever 1 - (1 - ci*ci) rounds to
                ec = __dmul_rn(eta, ci);
                const double ect = __dmul_rn(eta, ct);
                const double rs = __ddiv_rn(__dsub_rn(ec, ct), __dadd_rn(ec, ct)), rp = __ddiv_rn(__dsub_rn(ci, ect), __dadd_rn(ci, ect));
                const double F = __dmul_rn(__dadd_rn(__dmul_rn(rs, rs), __dmul_rn(rp, rp)), 0.5);
                if (a.fresnel && F > 0.0) {                             // (NaN: refracted, no draw)
                    const uint64_t id = id_of(a.ids, a.id_base, i);
                    refl = first_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kRefractDraw, a.k0, a.k1)) < F;
                }
                outcome = (inward ? 0 : 2) + (refl ? 1 : 0);
            }
            if (refl) {
                const double c2 = __dmul_rn(2.0, ci);
#pragma unroll
                for (int k = 0; k < 3; ++k) dir[k] = __dadd_rn(mh[k], __dmul_rn(c2, nf[k]));
            } else {
                const double g = __dsub_rn(ec, ct);
#pragma unroll
                for (int k = 0; k < 3; ++k) dir[k] = __dadd_rn(__dmul_rn(eta, mh[k]), __dmul_rn(g, nf[k]));
            }
            double y[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double vk = __dmul_rn(a.speed, dir[k]), drk = __dmul_rn(w, dir[k]), vo = (double)a.v[k][ti];
                y[k] = __dadd_rn(x[k], drk);
                a.r[k][ti] = (T)__dadd_rn(a.c[k], y[k]);
                a.v[k][ti] = (T)vk;
                a.dr[k][ti] = (T)drk;
                a.dv[k][ti] = (T)__dsub_rn(vk, vo);
            }
            const double q_new = dot3(y, y);                            // where the rest of the move has carried it (NaN: not counted)
            over = inward != refl ? q_new >= a.R2 : q_new < a.R2;       // in refracted and out reflected end inside, the others outside
        }
        if (__ballot(cross)) {  // (the same answer in every lane of the wave)
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const uint32_t n_k = (uint32_t)__popcll(__ballot(outcome == k));
                if (lane == 0 && n_k) atomicAdd(&s_cnt[k], n_k);
            }
            const uint32_t n_over = (uint32_t)__popcll(__ballot(over));
            if (lane == 0 && n_over) atomicAdd(&s_cnt[5], n_over);
        }
    }
    __syncthreads();
    // pcl_sweep::flush_cells, written out, for the reason given in k_absorb_scattered: a further caller changes the older kernels
    for (int k = threadIdx.x; k < 6; k += kBlock)
        if (s_cnt[k]) atomicAdd(&a.out[k], (unsigned long long)s_cnt[k]);
}

// The counter word of the draw that decides between the mirror and Lambert (the header lists who uses which word: 22 is this
// kernel's alone; the ground's own draws keep the ground's words 8 and 9).
constexpr uint32_t kSpectralMirrorDraw = 22;

template <typename T>
struct gspectral_args {
    T *r[3], *v[3], *dr[3], *dv[3];
    const T *E;
    const unsigned char *kind;   // NULL: every particle is a photon
    const int64_t *ids;          // NULL: the id of slot i is id_base + i
    const double *tables;        // albedo (B) | specular (B) | E edges (B + 1), device
    unsigned long long *out;     // reflected, absorbed, mirrored, out of band | reflected by band [B] | absorbed by band [B]; device, zeroed
    int64_t N, ts, id_base;      // particles, tile stride of the slab (elements), id of slot 0
    int tile_log;                // log2 of the tile length
    int n_E;                     // B >= 1
    double c[3], R2, speed;
    uint32_t k0, k1, pass;       // Philox key (seed_lo, seed_hi), the step's own pass counter
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_ground_spectral(gspectral_args<T> a) {
    extern __shared__ double s_mem[];                                  // albedo | specular | E edges | the four counts | by band, twice
    const int nE = a.n_E;
    const int n_tab = 3 * nE + 1, n_cells = 4 + 2 * nE;
    const double *s_alb = s_mem;
    const double *s_spec = s_alb + nE;
    const double *s_E = s_spec + nE;
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_mem + n_tab);
    uint32_t *s_refl = s_cnt + 4;
    uint32_t *s_gone = s_refl + nE;
    for (int k = threadIdx.x; k < n_tab; k += kBlock) s_mem[k] = a.tables[k];
    for (int k = threadIdx.x; k < n_cells; k += kBlock) s_cnt[k] = 0;  // (the bands' cells follow the four counts)
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = grid_stride(), n_round = whole_waves(a.N);   // (the ballots below need whole waves inside the loop)
    for (int64_t i = first_slot(); i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        double d[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0}, p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (in) {
                d[k] = __dsub_rn((double)a.r[k][ti], a.c[k]);           // fp32 widens exactly
                m[k] = (double)a.dr[k][ti];
            }
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = __dsub_rn(d[k], m[k]);
        const double q_now = dot3(d, d), q_prev = dot3(p, p);
        // the ground's hit (NaN: false)
        bool hit = in && q_now < a.R2 && q_prev >= a.R2 && q_prev < INFINITY;
        if (hit && a.kind) hit = a.kind[i] != 0;
        uint64_t id = 0;
        int band = -1;                                                  // -1: in no band, absorbed
        bool refl = false, mirror = false;
        if (hit) {
            const double e = (double)a.E[ti];                           // fp32 widens exactly
            if (e >= s_E[0] && e <= s_E[nE]) band = bin_of(s_E, nE, e); // (closed_bin: k_absorb_path's lookup) NaN and under/overflow: in no band
        }
        if (band >= 0) {
            const double alb = s_alb[band], sp = s_spec[band];
            id = id_of(a.ids, a.id_base, i);
            refl = true;
            if (alb < 1.0) refl = first_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, 9u, a.k0, a.k1)) < alb;   // the ground's draw
            mirror = refl && sp >= 1.0;
            if (refl && sp > 0.0 && sp < 1.0)
                mirror = first_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kSpectralMirrorDraw, a.k0, a.k1)) < sp;
        }
        const uint32_t n_hit = (uint32_t)__popcll(__ballot(hit)), n_refl = (uint32_t)__popcll(__ballot(refl));
        const uint32_t n_mirror = (uint32_t)__popcll(__ballot(mirror)), n_none = (uint32_t)__popcll(__ballot(hit && band < 0));
        if (lane == 0 && n_refl) atomicAdd(&s_cnt[0], n_refl);
        if (lane == 0 && n_hit - n_refl) atomicAdd(&s_cnt[1], n_hit - n_refl);
        if (lane == 0 && n_mirror) atomicAdd(&s_cnt[2], n_mirror);
        if (lane == 0 && n_none) atomicAdd(&s_cnt[3], n_none);
        if (!hit) continue;     // lanes that are not hit wait at the loop's head: no ballot below this line
        if (band >= 0) atomicAdd(refl ? &s_refl[band] : &s_gone[band], 1u);
        const double aq = dot3(m, m), b = dot3(p, m), cq = __dsub_rn(q_prev, a.R2);
        const double disc = fmax(__dsub_rn(__dmul_rn(b, b), __dmul_rn(aq, cq)), 0.0);
        const double t = __ddiv_rn(cq, __dsub_rn(__dsqrt_rn(disc), b));
        double x[3], nrm[3], vo[3], dir[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            x[k] = __dadd_rn(p[k], __dmul_rn(t, m[k]));
            vo[k] = (double)a.v[k][ti];
        }
        if (!refl) {            // absorbed: the ground's park, on the sphere, at rest
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                a.r[k][ti] = (T)__dadd_rn(a.c[k], x[k]);
                a.v[k][ti] = (T)0.0;
                a.dr[k][ti] = (T)__dsub_rn(x[k], p[k]);
                a.dv[k][ti] = (T)__dsub_rn(0.0, vo[k]);
            }
            continue;
        }
        const double xn = __dsqrt_rn(dot3(x, x)), sa = __dsqrt_rn(aq);
#pragma unroll
        for (int k = 0; k < 3; ++k) nrm[k] = __ddiv_rn(x[k], xn);
        if (mirror) {
            double mh[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) mh[k] = __ddiv_rn(m[k], sa);
            const double dn2 = __dmul_rn(2.0, dot3(mh, nrm));
#pragma unroll
            for (int k = 0; k < 3; ++k) dir[k] = __dsub_rn(mh[k], __dmul_rn(dn2, nrm[k]));
        } else {
            double u_a, u_b, sc, ss, e1[3], e2[3];
            pair_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, 8u, a.k0, a.k1), &u_a, &u_b);   // the ground's block
            const double mu = __dsqrt_rn(__dsub_rn(1.0, u_a));                                       // cosine-weighted hemisphere
            polar(mu, u_b, &sc, &ss);
            frame(nrm, e1, e2);
#pragma unroll
            for (int k = 0; k < 3; ++k) dir[k] = turned(sc, ss, mu, e1[k], e2[k], nrm[k]);
        }
        const double w = __dmul_rn(__dsub_rn(1.0, t), sa);              // the rest of the move, flown along the new direction
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double vk = __dmul_rn(a.speed, dir[k]), drk = __dmul_rn(w, dir[k]);
            a.r[k][ti] = (T)__dadd_rn(a.c[k], __dadd_rn(x[k], drk));
            a.v[k][ti] = (T)vk;
            a.dr[k][ti] = (T)drk;
            a.dv[k][ti] = (T)__dsub_rn(vk, vo[k]);
        }
    }
    __syncthreads();
    // pcl_sweep::flush_cells, written out, for the reason given in k_absorb_scattered: the count is not a literal
    for (int k = threadIdx.x; k < n_cells; k += kBlock)
        if (s_cnt[k]) atomicAdd(&a.out[k], (unsigned long long)s_cnt[k]);
}

struct surface_spec { // a call's arguments, checked
    double c[3] = {0.0, 0.0, 0.0};
    double R2 = 0.0, albedo = 1.0, speed = 0.0;
    int mode = PCL_SURFACE_LAMBERTIAN;
};

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.
bool check_spec(double radius, const double *center, double albedo, int mode, double c, const int64_t *counts_out, surface_spec &s) {
    if (!counts_out || (mode != PCL_SURFACE_LAMBERTIAN && mode != PCL_SURFACE_SPECULAR)) return false;
    s.R2 = radius * radius;
    if (!std::isfinite(radius) || !(radius > 0) || !std::isfinite(s.R2)) return false;
    if (!(albedo >= 0.0 && albedo <= 1.0) || !std::isfinite(c)) return false;
    if (center)
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(center[k])) return false;
            s.c[k] = center[k];
        }
    s.albedo = albedo; s.mode = mode; s.speed = c;
    return true;
}

template <typename T>
int launch_surface(pcl_ctx *ctx, const store_view &v, const surface_spec &s, uint64_t seed, uint32_t pass, const staged &st) {
    surface_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *vel = nullptr, *dr = nullptr, *dv = nullptr;
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &vel));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DR0 + k, &dr));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DV0 + k, &dv));
        a.r[k] = static_cast<T *>(r); a.v[k] = static_cast<T *>(vel);
        a.dr[k] = static_cast<T *>(dr); a.dv[k] = static_cast<T *>(dv);
        a.c[k] = s.c[k];
    }
    a.kind = st.kind; a.ids = st.ids; a.out = st.out;
    a.N = v.N; a.ts = v.ts; a.id_base = st.id_base; a.tile_log = v.tile_log; a.mode = s.mode;
    a.R2 = s.R2; a.albedo = s.albedo; a.speed = s.speed;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.pass = pass;
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(2 * sizeof(uint32_t)));
    hipLaunchKernelGGL(k_surface_reflect<T>, dim3((unsigned)grid), dim3(kBlock), 0, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int surface_reflect(pcl_ctx *ctx, double radius, const double *center_host, double albedo, int mode, double c, uint64_t seed,
                    uint32_t pass, int64_t *counts_out_host) {
    surface_spec s;
    if (!ctx || !check_spec(radius, center_host, albedo, mode, c, counts_out_host, s)) return bad_argument(ctx);
    // E is never asked for: the pointer costs a wavelength-dependent scatter step its term cache (pcl_shell.hip).
    const spans out = {{counts_out_host, 2}};
    store_view v;
    staged st(ctx);
    PCL_SWEEP_TRY(open_store(ctx, PCL_R0, &v));
    zero_spans(out);
    if (v.N <= 0) return PCL_OK;
    PCL_SWEEP_TRY(stage(st, v, 2, nullptr, 0, true));
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_surface, ctx, v, s, seed, pass, st));
    return fetch(st, out);
}

int group_surface_reflect(pcl_group *group, double radius, const double *center_host, double albedo, int mode, double c,
                          uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    const int n = (int)ctx.size();
    surface_spec s;
    if (n < 1 || !check_spec(radius, center_host, albedo, mode, c, counts_out_host, s)) return bad_argument(n > 0 ? ctx[0] : nullptr);
    return sum_shards(ctx, {{counts_out_host, 2}}, [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_surface_reflect(one, radius, center_host, albedo, mode, c, seed, pass, p);
    });
}

// Everything PCL_ERR_ARG stands for except the NULL context (g is looked at for Henyey-Greenstein only)
bool check_phase(int phase, double g, double c, const int64_t *count_out) {
    if (!count_out || (phase != PCL_PHASE_ISOTROPIC && phase != PCL_PHASE_HG && phase != PCL_PHASE_RAYLEIGH)) return false;
    if (phase == PCL_PHASE_HG && !(std::isfinite(g) && std::fabs(g) < 1.0)) return false;
    return std::isfinite(c);
}

template <typename T>
int launch_phase(pcl_ctx *ctx, const store_view &v, int phase, double g, double c, uint64_t seed, uint32_t pass,
                 const staged &st) {
    phase_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *vel = nullptr, *dv = nullptr;
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &vel));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DV0 + k, &dv));     // (what makes a lazy dv real)
        a.v[k] = static_cast<T *>(vel); a.dv[k] = static_cast<T *>(dv);
    }
    a.kind = st.kind; a.ids = st.ids; a.out = st.out;
    a.N = v.N; a.ts = v.ts; a.id_base = st.id_base; a.tile_log = v.tile_log; a.phase = phase;
    a.g = g; a.speed = c;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.pass = pass;
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(sizeof(uint32_t)));
    hipLaunchKernelGGL(k_phase_redirect<T>, dim3((unsigned)grid), dim3(kBlock), 0, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int phase_redirect(pcl_ctx *ctx, int phase, double g, double c, uint64_t seed, uint32_t pass, int64_t *count_out_host) {
    if (!ctx || !check_phase(phase, g, c, count_out_host)) return bad_argument(ctx);
    const spans out = {{count_out_host, 1}};
    store_view v;                                                       // E is never asked for, as above
    staged st(ctx);
    PCL_SWEEP_TRY(open_store(ctx, PCL_DV0, &v));
    zero_spans(out);
    if (v.N <= 0) return PCL_OK;
    PCL_SWEEP_TRY(stage(st, v, 1, nullptr, 0, true));
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_phase, ctx, v, phase, g, c, seed, pass, st));
    return fetch(st, out);
}

int group_phase_redirect(pcl_group *group, int phase, double g, double c, uint64_t seed, uint32_t pass, int64_t *count_out_host) {
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    const int n = (int)ctx.size();
    if (n < 1 || !check_phase(phase, g, c, count_out_host)) return bad_argument(n > 0 ? ctx[0] : nullptr);
    return sum_shards(ctx, {{count_out_host, 1}}, [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_phase_redirect(one, phase, g, c, seed, pass, p);
    });
}

struct absorb_spec { // a call's arguments, checked; what the kernel compares against
    int n_layers = 0, n_E = 0;
    double c[3] = {0.0, 0.0, 0.0};
    bool draws = false;         // some layer has omega0 < 1: the ids are needed
    std::vector<double> tables; // omega0 | e*e | E edges
    int rows() const { return n_layers > 0 ? n_layers : 1; }
    size_t cells() const { return (size_t)2 + (size_t)rows() * (1 + (size_t)n_E); }
    spans out(int64_t *counts, int64_t *E_hist) const { return {{counts, (size_t)2 + rows()}, {E_hist, (size_t)rows() * n_E}}; }
};

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.
bool check_absorb(int n_layers, const double *omega0, const double *edges, const double *center, int n_E, const double *E_edges,
                  const int64_t *counts_out, const int64_t *E_hist_out, absorb_spec &s) {
    if (!omega0 || !counts_out || n_layers < 0 || n_layers > PCL_ABSORB_MAX_LAYERS) return false;
    if (n_E < 0 || n_E > PCL_ABSORB_MAX_BINS || (n_E > 0 && (!E_edges || !E_hist_out))) return false;
    s.n_layers = n_layers; s.n_E = n_E;
    if (s.cells() > PCL_ABSORB_MAX_CELLS) return false;                 // the workgroup's cells and tables stay below 64 KiB of LDS
    for (int b = 0; b < s.rows(); ++b) {
        if (!(omega0[b] >= 0.0 && omega0[b] <= 1.0)) return false;      // (NaN as well)
        s.draws = s.draws || omega0[b] < 1.0;
        s.tables.push_back(omega0[b]);
    }
    if (n_layers > 0 && (!edges || !check_edges(edges, n_layers, kEdgeSquare, &s.tables))) return false;
    if (n_E > 0 && !check_edges(E_edges, n_E, kEdgePlain, &s.tables)) return false;
    if (center)
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(center[k])) return false;
            s.c[k] = center[k];
        }
    return true;
}

template <typename T>
int launch_absorb(pcl_ctx *ctx, const store_view &v, const absorb_spec &s, const void *E, uint64_t seed, uint32_t pass,
                  const staged &st) {
    absorb_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *vel = nullptr, *dv = nullptr;
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &vel));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DV0 + k, &dv));
        a.r[k] = static_cast<const T *>(r); a.v[k] = static_cast<T *>(vel); a.dv[k] = static_cast<T *>(dv);
        a.c[k] = s.c[k];
    }
    a.E = static_cast<const T *>(E); a.kind = st.kind; a.ids = st.ids; a.tables = st.tables; a.out = st.out;
    a.N = v.N; a.ts = v.ts; a.id_base = st.id_base; a.tile_log = v.tile_log;
    a.n_layers = s.n_layers; a.n_E = s.n_E;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.pass = pass;
    const size_t lds = s.tables.size() * sizeof(double) + s.cells() * sizeof(uint32_t);
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(lds));
    hipLaunchKernelGGL(k_absorb_scattered<T>, dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int absorb_scattered(pcl_ctx *ctx, int n_layers, const double *omega0_host, const double *edges_host, const double *center_host,
                     int n_E_bins, const double *E_edges_host, uint64_t seed, uint32_t pass, int64_t *counts_out_host,
                     int64_t *E_hist_out_host) {
    absorb_spec s;
    if (!ctx || !check_absorb(n_layers, omega0_host, edges_host, center_host, n_E_bins, E_edges_host, counts_out_host, E_hist_out_host, s))
        return bad_argument(ctx);
    const spans out = s.out(counts_out_host, E_hist_out_host);
    store_view v;
    staged st(ctx);
    PCL_SWEEP_TRY(open_store(ctx, PCL_DV0, &v));
    zero_spans(out);
    if (v.N <= 0) return PCL_OK;
    // E is asked for only with energy bins: the pointer costs a wavelength-dependent scatter step its term cache (pcl_shell.hip).
    void *E = nullptr;
    if (s.n_E) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_E, &E));
    PCL_SWEEP_TRY(stage(st, v, s.cells(), s.tables.data(), s.tables.size(), s.draws));   // the ids only if somebody may draw
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_absorb, ctx, v, s, E, seed, pass, st));
    return fetch(st, out);
}

int group_absorb_scattered(pcl_group *group, int n_layers, const double *omega0_host, const double *edges_host, const double *center_host,
                           int n_E_bins, const double *E_edges_host, uint64_t seed, uint32_t pass, int64_t *counts_out_host,
                           int64_t *E_hist_out_host) {
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    const int n = (int)ctx.size();
    absorb_spec s;
    if (n < 1 || !check_absorb(n_layers, omega0_host, edges_host, center_host, n_E_bins, E_edges_host, counts_out_host, E_hist_out_host, s))
        return bad_argument(n > 0 ? ctx[0] : nullptr);
    return sum_shards(ctx, s.out(counts_out_host, E_hist_out_host), [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_absorb_scattered(one, n_layers, omega0_host, edges_host, center_host, n_E_bins, E_edges_host, seed, pass, p,
                                         n_E_bins ? p + 2 + s.rows() : nullptr);
    });
}

struct lphase_spec { // a call's arguments, checked; what the kernel reads
    int n_layers = 0, n_laws = 0, n_nodes = 0;
    double c[3] = {0.0, 0.0, 0.0};
    double speed = 0.0;
    std::vector<double> tables; // C | e*e | g | mu | F | s | the laws' ints
    int rows() const { return n_layers > 0 ? n_layers : 1; }
    size_t cells() const { return (size_t)2 + (size_t)rows() + (size_t)n_laws; }
    size_t lds() const { return tables.size() * sizeof(double) + cells() * sizeof(uint32_t); }
};

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.
bool check_lphase(int n_laws, const int *kinds, const double *g, const int *n_bins, const double *mu, const double *F, int n_layers,
                  const double *cum, const double *edges, const double *center, double c, const int64_t *counts_out, lphase_spec &s) {
    if (!kinds || !cum || !counts_out || n_laws < 1 || n_laws > PCL_LPHASE_MAX_LAWS) return false;
    if (n_layers < 0 || n_layers > PCL_LPHASE_MAX_LAYERS || !std::isfinite(c)) return false;
    s.n_layers = n_layers; s.n_laws = n_laws; s.speed = c;
    const int M = n_laws;
    for (int b = 0; b < s.rows(); ++b) {                                // a row of C: cumulative, from >= 0 up to exactly 1
        double prev = 0.0;
        for (int j = 0; j < M; ++j) {
            const double x = cum[(size_t)b * M + j];
            if (!(x >= prev && x <= 1.0)) return false;                 // (NaN as well)
            s.tables.push_back(prev = x);
        }
        if (prev != 1.0) return false;
    }
    if (n_layers > 0 && (!edges || !check_edges(edges, n_layers, kEdgeSquare, &s.tables))) return false;
    std::vector<int> ints((size_t)3 * M, 0);                            // kind | first node | bins
    int64_t total_bins = 0;
    for (int j = 0; j < M; ++j) {
        const int kind = kinds[j];
        double gj = 0.0;
        if (kind == PCL_PHASE_HG) {
            if (!g || !(std::isfinite(g[j]) && std::fabs(g[j]) < 1.0)) return false;
            gj = g[j];
        } else if (kind == PCL_PHASE_TABLE) {
            if (!n_bins || !mu || !F || n_bins[j] < 1 || n_bins[j] > PCL_LPHASE_MAX_NODES) return false;
            total_bins += n_bins[j];
        } else if (kind != PCL_PHASE_ISOTROPIC && kind != PCL_PHASE_RAYLEIGH) {
            return false;
        }
        ints[(size_t)j] = kind;
        s.tables.push_back(gj);
    }
    if (total_bins > PCL_LPHASE_MAX_TOTAL_NODES) return false;
    std::vector<double> nodes, cumul, slope;
    for (int j = 0; j < M; ++j) {
        if (kinds[j] != PCL_PHASE_TABLE) continue;
        const int K = n_bins[j];
        const size_t at = nodes.size();                                 // the tables' nodes follow one another, in the order of the laws
        ints[(size_t)M + j] = (int)at;
        ints[(size_t)2 * M + j] = K;
        const double *m = mu + at, *f = F + at;
        if (m[0] != -1.0 || m[K] != 1.0 || f[0] != 0.0 || f[K] != 1.0) return false;
        for (int k = 0; k <= K; ++k) {
            if (k > 0 && (!(m[k] > m[k - 1]) || !(f[k] > f[k - 1]))) return false;       // (NaN as well)
            nodes.push_back(m[k]);
            cumul.push_back(f[k]);
            const double sl = k < K ? (m[k + 1] - m[k]) / (f[k + 1] - f[k]) : 0.0;       // one rounding each; the last node has no bin
            if (!std::isfinite(sl)) return false;
            slope.push_back(sl);
        }
    }
    s.n_nodes = (int)nodes.size();
    s.tables.insert(s.tables.end(), nodes.begin(), nodes.end());
    s.tables.insert(s.tables.end(), cumul.begin(), cumul.end());
    s.tables.insert(s.tables.end(), slope.begin(), slope.end());
    const size_t n_dbl = s.tables.size();
    s.tables.resize(n_dbl + ((size_t)3 * M + 1) / 2, 0.0);
    memcpy(s.tables.data() + n_dbl, ints.data(), ints.size() * sizeof(int));
    if (s.lds() >= (size_t)64 * 1024) return false;                    // the workgroup's tables and cells stay below 64 KiB of LDS
    if (center)
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(center[k])) return false;
            s.c[k] = center[k];
        }
    return true;
}

template <typename T>
int launch_lphase(pcl_ctx *ctx, const store_view &v, const lphase_spec &s, uint64_t seed, uint32_t pass, const staged &st) {
    lphase_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *vel = nullptr, *dv = nullptr;
        if (s.n_layers > 0) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &vel));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DV0 + k, &dv));
        a.r[k] = static_cast<const T *>(r); a.v[k] = static_cast<T *>(vel); a.dv[k] = static_cast<T *>(dv);
        a.c[k] = s.c[k];
    }
    a.kind = st.kind; a.ids = st.ids; a.tables = st.tables; a.out = st.out;
    a.N = v.N; a.ts = v.ts; a.id_base = st.id_base; a.tile_log = v.tile_log;
    a.n_layers = s.n_layers; a.n_laws = s.n_laws; a.n_nodes = s.n_nodes; a.speed = s.speed;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.pass = pass;
    const size_t lds = s.lds();                                         // what this call uses: a few hundred bytes without a table
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(lds));
    hipLaunchKernelGGL(k_phase_layered<T>, dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int phase_layered(pcl_ctx *ctx, int n_laws, const int *kinds, const double *g, const int *n_bins, const double *mu, const double *F,
                  int n_layers, const double *cum, const double *edges, const double *center, double c, uint64_t seed, uint32_t pass,
                  int64_t *counts_out_host) {
    lphase_spec s;
    if (!ctx || !check_lphase(n_laws, kinds, g, n_bins, mu, F, n_layers, cum, edges, center, c, counts_out_host, s)) return bad_argument(ctx);
    const spans out = {{counts_out_host, s.cells()}};
    store_view v;                                                       // E is never asked for, as in phase_redirect
    staged st(ctx);
    PCL_SWEEP_TRY(open_store(ctx, PCL_DV0, &v));
    zero_spans(out);
    if (v.N <= 0) return PCL_OK;
    PCL_SWEEP_TRY(stage(st, v, s.cells(), s.tables.data(), s.tables.size(), true));
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_lphase, ctx, v, s, seed, pass, st));
    return fetch(st, out);
}

int group_phase_layered(pcl_group *group, int n_laws, const int *kinds, const double *g, const int *n_bins, const double *mu,
                        const double *F, int n_layers, const double *cum, const double *edges, const double *center, double c,
                        uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    const int n = (int)ctx.size();
    lphase_spec s;
    if (n < 1 || !check_lphase(n_laws, kinds, g, n_bins, mu, F, n_layers, cum, edges, center, c, counts_out_host, s))
        return bad_argument(n > 0 ? ctx[0] : nullptr);
    return sum_shards(ctx, {{counts_out_host, s.cells()}}, [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_phase_layered(one, n_laws, kinds, g, n_bins, mu, F, n_layers, cum, edges, center, c, seed, pass, p);
    });
}

struct recycle_spec { // a call's arguments, checked
    double c[3] = {0.0, 0.0, 0.0};
    double top2 = 0.0, speed = 0.0;
    bool at_rest = false, has_top = false;
    int n_E = 0;
    std::vector<double> tables; // cdf | grid
    size_t lds() const { return tables.size() * sizeof(double) + 2 * sizeof(uint32_t); }
};

bool finite3(const double *x) { return std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]); }

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.  The source
// is checked as pcl_store_apply_source checks it.
bool check_recycle(const pcl_source *src, double c, int at_rest, double top, const double *center, int n_E, const double *cdf,
                   const double *grid, const int64_t *counts_out, recycle_spec &s) {
    if (!src || !counts_out) return false;
    if (src->angular < PCL_SRC_BEAM || src->angular > PCL_SRC_LAMBERTIAN || src->spatial < PCL_SRC_POINT || src->spatial > PCL_SRC_GAUSSIAN)
        return false;
    if (!finite3(src->origin) || !finite3(src->e1) || !finite3(src->e2) || !finite3(src->d) || !std::isfinite(c)) return false;
    if (src->angular == PCL_SRC_CONE && !(src->cos_half_angle >= -1.0 && src->cos_half_angle <= 1.0)) return false;
    if (src->spatial != PCL_SRC_POINT && !(std::isfinite(src->radius) && src->radius >= 0.0)) return false;
    if (!std::isfinite(top)) return false;
    s.at_rest = at_rest != 0; s.has_top = top > 0.0; s.speed = c;
    if (s.has_top && !std::isfinite(s.top2 = top * top)) return false;
    if (!s.at_rest && !s.has_top) return false;                         // neither criterion: nobody could ever be spent
    if (center) {
        if (!finite3(center)) return false;
        for (int k = 0; k < 3; ++k) s.c[k] = center[k];
    }
    if (n_E < 0 || n_E > PCL_RECYCLE_MAX_BINS || (n_E > 0 && (!cdf || !grid))) return false;
    s.n_E = n_E;
    double prev = -INFINITY;
    for (int k = 0; k < n_E; ++k) {
        if (!(cdf[k] >= prev)) return false;                            // (NaN as well)
        s.tables.push_back(prev = cdf[k]);
    }
    if (n_E > 0 && prev != 1.0) return false;
    for (int k = 0; k < n_E; ++k) {
        if (!std::isfinite(grid[k])) return false;
        s.tables.push_back(grid[k]);
    }
    return true;
}

template <typename T>
int launch_recycle(pcl_ctx *ctx, const store_view &v, const recycle_spec &s, const pcl_source *src, uint64_t seed, uint32_t pass,
                   const staged &st) {
    recycle_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *vel = nullptr, *dr = nullptr, *dv = nullptr;
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &vel));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DR0 + k, &dr));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DV0 + k, &dv));
        a.r[k] = static_cast<T *>(r); a.v[k] = static_cast<T *>(vel);
        a.dr[k] = static_cast<T *>(dr); a.dv[k] = static_cast<T *>(dv);
        a.c[k] = s.c[k];
        a.origin[k] = src->origin[k]; a.e1[k] = src->e1[k]; a.e2[k] = src->e2[k]; a.d[k] = src->d[k];
    }
    // E is asked for only with a spectrum: the pointer costs a wavelength-dependent scatter step its term cache (pcl_shell.hip).
    void *E = nullptr;
    if (s.n_E > 0) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_E, &E));
    a.E = static_cast<T *>(E); a.kind = st.kind; a.ids = st.ids; a.tables = st.tables; a.out = st.out;
    a.N = v.N; a.ts = v.ts; a.id_base = st.id_base; a.tile_log = v.tile_log;
    a.at_rest = s.at_rest; a.has_top = s.has_top; a.n_E = s.n_E; a.angular = src->angular; a.spatial = src->spatial;
    a.top2 = s.top2; a.speed = s.speed; a.cos_half_angle = src->cos_half_angle; a.radius = src->radius;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.pass = pass;
    const size_t lds = s.lds();                                         // 16 KiB of tables at the most: eight workgroups a CU still
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(lds));
    hipLaunchKernelGGL(k_recycle_spent<T>, dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int recycle_spent(pcl_ctx *ctx, const pcl_source *src, double c, int at_rest, double top, const double *center_host, int n_E,
                  const double *cdf_host, const double *grid_host, uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    recycle_spec s;
    if (!ctx || !check_recycle(src, c, at_rest, top, center_host, n_E, cdf_host, grid_host, counts_out_host, s)) return bad_argument(ctx);
    const spans out = {{counts_out_host, 2}};
    store_view v;
    staged st(ctx);
    PCL_SWEEP_TRY(open_store(ctx, PCL_R0, &v));
    zero_spans(out);
    if (v.N <= 0) return PCL_OK;
    PCL_SWEEP_TRY(stage(st, v, 2, s.tables.data(), s.tables.size(), true));
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_recycle, ctx, v, s, src, seed, pass, st));
    return fetch(st, out);
}

int group_recycle_spent(pcl_group *group, const pcl_source *src, double c, int at_rest, double top, const double *center_host, int n_E,
                        const double *cdf_host, const double *grid_host, uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    const int n = (int)ctx.size();
    recycle_spec s;
    if (n < 1 || !check_recycle(src, c, at_rest, top, center_host, n_E, cdf_host, grid_host, counts_out_host, s))
        return bad_argument(n > 0 ? ctx[0] : nullptr);
    return sum_shards(ctx, {{counts_out_host, 2}}, [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_recycle_spent(one, src, c, at_rest, top, center_host, n_E, cdf_host, grid_host, seed, pass, p);
    });
}

struct pabsorb_spec { // a call's arguments, checked; what the kernel compares against
    int n_layers = 0, n_E = 0;
    double c[3] = {0.0, 0.0, 0.0};
    bool draws = false;         // some cell has p > 0: the ids are needed
    std::vector<double> tables; // p | e*e | E edges
    size_t rows() const { return n_layers > 0 ? (size_t)n_layers : 1; }
    size_t cols() const { return n_E > 0 ? (size_t)n_E : 1; }
    size_t cells() const { return (size_t)2 + rows() * cols(); }       // exposed, absorbed | by cell
    size_t lds() const { return tables.size() * sizeof(double) + cells() * sizeof(uint32_t); }
    spans out(int64_t *counts, int64_t *by_cell) const { return {{counts, 2}, {by_cell, cells() - 2}}; }
};

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.
bool check_pabsorb(int n_layers, int n_E, const double *p, const double *edges, const double *center, const double *E_edges,
                   const int64_t *counts_out, const int64_t *cells_out, pabsorb_spec &s) {
    if (!p || !counts_out || !cells_out || n_layers < 0 || n_layers > PCL_PATH_ABSORB_MAX_LAYERS) return false;
    if (n_E < 0 || n_E > PCL_PATH_ABSORB_MAX_BANDS) return false;
    s.n_layers = n_layers; s.n_E = n_E;
    const size_t n_p = s.rows() * s.cols();
    if (n_p > PCL_PATH_ABSORB_MAX_CELLS) return false;                  // the workgroup's cells and tables stay below 64 KiB of LDS
    for (size_t k = 0; k < n_p; ++k) {
        if (!(p[k] >= 0.0 && p[k] <= 1.0)) return false;                // (NaN as well)
        s.draws = s.draws || p[k] > 0.0;
        s.tables.push_back(p[k]);
    }
    if (n_layers > 0 && (!edges || !check_edges(edges, n_layers, kEdgeSquare, &s.tables))) return false;
    if (n_E > 0 && (!E_edges || !check_edges(E_edges, n_E, kEdgePlain, &s.tables))) return false;
    if (center)
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(center[k])) return false;
            s.c[k] = center[k];
        }
    return true;
}

template <typename T>
int launch_pabsorb(pcl_ctx *ctx, const store_view &v, const pabsorb_spec &s, uint64_t seed, uint32_t pass, const staged &st) {
    pabsorb_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *vel = nullptr, *dv = nullptr;
        if (s.n_layers > 0) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &vel));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DV0 + k, &dv));     // (what makes a lazy dv real: an absorbed photon's is written)
        a.r[k] = static_cast<const T *>(r); a.v[k] = static_cast<T *>(vel); a.dv[k] = static_cast<T *>(dv);
        a.c[k] = s.c[k];
    }
    // E is asked for only with energy bands: the pointer costs a wavelength-dependent scatter step its term cache (pcl_shell.hip).
    void *E = nullptr;
    if (s.n_E > 0) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_E, &E));
    a.E = static_cast<const T *>(E); a.kind = st.kind; a.ids = st.ids; a.tables = st.tables; a.out = st.out;
    a.N = v.N; a.ts = v.ts; a.id_base = st.id_base; a.tile_log = v.tile_log;
    a.n_layers = s.n_layers; a.n_E = s.n_E;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.pass = pass;
    const size_t lds = s.lds();                                         // what this call uses: 24 B for a grey gas everywhere
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(lds));
    hipLaunchKernelGGL(k_absorb_path<T>, dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int absorb_path(pcl_ctx *ctx, int n_layers, int n_E_bins, const double *p_host, const double *edges_host, const double *center_host,
                const double *E_edges_host, uint64_t seed, uint32_t pass, int64_t *counts_out_host, int64_t *cells_out_host) {
    pabsorb_spec s;
    if (!ctx || !check_pabsorb(n_layers, n_E_bins, p_host, edges_host, center_host, E_edges_host, counts_out_host, cells_out_host, s))
        return bad_argument(ctx);
    const spans out = s.out(counts_out_host, cells_out_host);
    store_view v;
    staged st(ctx);
    PCL_SWEEP_TRY(open_store(ctx, PCL_V0, &v));
    zero_spans(out);
    if (v.N <= 0) return PCL_OK;
    PCL_SWEEP_TRY(stage(st, v, s.cells(), s.tables.data(), s.tables.size(), s.draws));   // the ids only if somebody may draw
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_pabsorb, ctx, v, s, seed, pass, st));
    return fetch(st, out);
}

int group_absorb_path(pcl_group *group, int n_layers, int n_E_bins, const double *p_host, const double *edges_host,
                      const double *center_host, const double *E_edges_host, uint64_t seed, uint32_t pass, int64_t *counts_out_host,
                      int64_t *cells_out_host) {
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    const int n = (int)ctx.size();
    pabsorb_spec s;
    if (n < 1 || !check_pabsorb(n_layers, n_E_bins, p_host, edges_host, center_host, E_edges_host, counts_out_host, cells_out_host, s))
        return bad_argument(n > 0 ? ctx[0] : nullptr);
    return sum_shards(ctx, s.out(counts_out_host, cells_out_host), [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_absorb_path(one, n_layers, n_E_bins, p_host, edges_host, center_host, E_edges_host, seed, pass, p, p + 2);
    });
}

struct reemit_spec { // a call's arguments, checked; what the kernel reads
    int n_layers = 0, n_bins = 0;
    double c[3] = {0.0, 0.0, 0.0};
    double speed = 0.0;
    bool draws = false;         // some layer has eta > 0: the ids are needed
    bool need_r = false;        // layers, or a lambertian layer
    std::vector<double> tables; // eta | e*e | cdf | grid | the layers' ints
    size_t rows() const { return n_layers > 0 ? (size_t)n_layers : 1; }
    size_t cells() const { return (size_t)2 + rows(); }                // parked, re-emitted | by layer
    size_t lds() const { return tables.size() * sizeof(double) + cells() * sizeof(uint32_t); }
};

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.
bool check_reemit(int n_layers, const double *edges, const double *center, const double *eta, const int *lambertian, const int *offsets,
                  const double *cdf, const double *grid, double c, const int64_t *counts_out, reemit_spec &s) {
    if (!eta || !lambertian || !offsets || !counts_out || n_layers < 0 || n_layers > PCL_REEMIT_MAX_LAYERS || !std::isfinite(c)) return false;
    s.n_layers = n_layers; s.speed = c; s.need_r = n_layers > 0;
    const size_t Lp = s.rows();
    for (size_t b = 0; b < Lp; ++b) {
        if (!(eta[b] >= 0.0 && eta[b] <= 1.0)) return false;            // (NaN as well)
        if (lambertian[b] != 0 && lambertian[b] != 1) return false;
        s.draws = s.draws || eta[b] > 0.0;
        s.need_r = s.need_r || lambertian[b] == 1;
        s.tables.push_back(eta[b]);
    }
    if (n_layers > 0 && (!edges || !check_edges(edges, n_layers, kEdgeSquare, &s.tables))) return false;
    if (offsets[0] != 0) return false;
    for (size_t b = 0; b < Lp; ++b) {                                   // equal neighbours: the layer has no table
        const int64_t bins = (int64_t)offsets[b + 1] - offsets[b];
        if (bins < 0 || bins > PCL_REEMIT_MAX_BINS || offsets[b + 1] > PCL_REEMIT_MAX_TOTAL_BINS) return false;
    }
    s.n_bins = offsets[Lp];
    if (s.n_bins > 0 && (!cdf || !grid)) return false;
    for (size_t b = 0; b < Lp; ++b) {                                   // each table as pcl_step_recycle_spent checks its one
        double prev = -INFINITY;
        for (int k = offsets[b]; k < offsets[b + 1]; ++k) {
            if (!(cdf[k] >= prev)) return false;                        // (NaN as well)
            s.tables.push_back(prev = cdf[k]);
        }
        if (offsets[b + 1] > offsets[b] && prev != 1.0) return false;
    }
    for (int k = 0; k < s.n_bins; ++k) {
        if (!std::isfinite(grid[k])) return false;
        s.tables.push_back(grid[k]);
    }
    std::vector<int> ints;                                              // lambertian (L') | offsets (L' + 1)
    ints.insert(ints.end(), lambertian, lambertian + Lp);
    ints.insert(ints.end(), offsets, offsets + Lp + 1);
    const size_t n_dbl = s.tables.size();
    s.tables.resize(n_dbl + (2 * Lp + 2) / 2, 0.0);
    memcpy(s.tables.data() + n_dbl, ints.data(), ints.size() * sizeof(int));
    if (center) {
        if (!finite3(center)) return false;
        for (int k = 0; k < 3; ++k) s.c[k] = center[k];
    }
    return true;
}

template <typename T>
int launch_reemit(pcl_ctx *ctx, const store_view &v, const reemit_spec &s, uint64_t seed, uint32_t pass, const staged &st) {
    reemit_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *vel = nullptr, *dr = nullptr, *dv = nullptr;
        if (s.need_r) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &vel));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DR0 + k, &dr));     // (what makes an implicit dr and a lazy dv real: a re-emitted
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DV0 + k, &dv));     //  photon's are written)
        a.r[k] = static_cast<const T *>(r); a.v[k] = static_cast<T *>(vel);
        a.dr[k] = static_cast<T *>(dr); a.dv[k] = static_cast<T *>(dv);
        a.c[k] = s.c[k];
    }
    // E is asked for only if a layer has a table: the pointer costs a wavelength-dependent scatter step its term cache (pcl_shell.hip).
    void *E = nullptr;
    if (s.n_bins > 0) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_E, &E));
    a.E = static_cast<T *>(E); a.kind = st.kind; a.ids = st.ids; a.tables = st.tables; a.out = st.out;
    a.N = v.N; a.ts = v.ts; a.id_base = st.id_base; a.tile_log = v.tile_log;
    a.n_layers = s.n_layers; a.n_bins = s.n_bins; a.need_r = s.need_r; a.speed = s.speed;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.pass = pass;
    const size_t lds = s.lds();                                         // 34 KiB with the largest tables: four workgroups a CU still
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(lds));
    hipLaunchKernelGGL(k_reemit_parked<T>, dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int reemit_parked(pcl_ctx *ctx, int n_layers, const double *edges_host, const double *center_host, const double *eta_host,
                  const int *lambertian_host, const int *table_offsets_host, const double *cdf_host, const double *grid_host, double c,
                  uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    reemit_spec s;
    if (!ctx || !check_reemit(n_layers, edges_host, center_host, eta_host, lambertian_host, table_offsets_host, cdf_host, grid_host, c,
                              counts_out_host, s))
        return bad_argument(ctx);
    const spans out = {{counts_out_host, s.cells()}};
    store_view v;
    staged st(ctx);
    PCL_SWEEP_TRY(open_store(ctx, PCL_V0, &v));
    zero_spans(out);
    if (v.N <= 0) return PCL_OK;
    PCL_SWEEP_TRY(stage(st, v, s.cells(), s.tables.data(), s.tables.size(), s.draws));   // the ids only if somebody may draw
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_reemit, ctx, v, s, seed, pass, st));
    return fetch(st, out);
}

int group_reemit_parked(pcl_group *group, int n_layers, const double *edges_host, const double *center_host, const double *eta_host,
                        const int *lambertian_host, const int *table_offsets_host, const double *cdf_host, const double *grid_host,
                        double c, uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    const int n = (int)ctx.size();
    reemit_spec s;
    if (n < 1 || !check_reemit(n_layers, edges_host, center_host, eta_host, lambertian_host, table_offsets_host, cdf_host, grid_host, c,
                               counts_out_host, s))
        return bad_argument(n > 0 ? ctx[0] : nullptr);
    return sum_shards(ctx, {{counts_out_host, s.cells()}}, [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_reemit_parked(one, n_layers, edges_host, center_host, eta_host, lambertian_host, table_offsets_host, cdf_host,
                                      grid_host, c, seed, pass, p);
    });
}

struct refract_spec { // a call's arguments, checked; the two ratios are made here, once
    double c[3] = {0.0, 0.0, 0.0};
    double R2 = 0.0, eta_in = 1.0, eta_out = 1.0, speed = 0.0;
    bool fresnel = true;
};

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.
bool check_refract(double radius, const double *center, double n_inside, double n_outside, int fresnel, double c, const int64_t *counts_out,
                   refract_spec &s) {
    if (!counts_out) return false;
    s.R2 = radius * radius;
    if (!std::isfinite(radius) || !(radius > 0) || !std::isfinite(s.R2)) return false;
    if (!std::isfinite(n_inside) || !(n_inside > 0) || !std::isfinite(n_outside) || !(n_outside > 0) || !std::isfinite(c)) return false;
    if (center) {
        if (!finite3(center)) return false;
        for (int k = 0; k < 3; ++k) s.c[k] = center[k];
    }
    s.eta_in = n_outside / n_inside; s.eta_out = n_inside / n_outside;   // one rounding each
    s.fresnel = fresnel != 0; s.speed = c;
    return true;
}

template <typename T>
int launch_refract(pcl_ctx *ctx, const store_view &v, const refract_spec &s, uint64_t seed, uint32_t pass, const staged &st) {
    refract_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *vel = nullptr, *dr = nullptr, *dv = nullptr;
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &vel));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DR0 + k, &dr));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DV0 + k, &dv));
        a.r[k] = static_cast<T *>(r); a.v[k] = static_cast<T *>(vel);
        a.dr[k] = static_cast<T *>(dr); a.dv[k] = static_cast<T *>(dv);
        a.c[k] = s.c[k];
    }
    a.kind = st.kind; a.ids = st.ids; a.out = st.out;
    a.N = v.N; a.ts = v.ts; a.id_base = st.id_base; a.tile_log = v.tile_log; a.fresnel = s.fresnel;
    a.R2 = s.R2; a.eta_in = s.eta_in; a.eta_out = s.eta_out; a.speed = s.speed;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.pass = pass;
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(6 * sizeof(uint32_t)));
    hipLaunchKernelGGL(k_refract_surface<T>, dim3((unsigned)grid), dim3(kBlock), 0, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int refract_surface(pcl_ctx *ctx, double radius, const double *center_host, double n_inside, double n_outside, int fresnel, double c,
                    uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    refract_spec s;
    if (!ctx || !check_refract(radius, center_host, n_inside, n_outside, fresnel, c, counts_out_host, s)) return bad_argument(ctx);
    const spans out = {{counts_out_host, 6}};
    store_view v;                                                       // E is never asked for, as in surface_reflect
    staged st(ctx);
    PCL_SWEEP_TRY(open_store(ctx, PCL_R0, &v));
    zero_spans(out);
    if (v.N <= 0) return PCL_OK;
    PCL_SWEEP_TRY(stage(st, v, 6, nullptr, 0, s.fresnel));              // the ids only if somebody may draw
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_refract, ctx, v, s, seed, pass, st));
    return fetch(st, out);
}

int group_refract_surface(pcl_group *group, double radius, const double *center_host, double n_inside, double n_outside, int fresnel,
                          double c, uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    refract_spec s;                                                     // the arguments first: a refused call looks at no group
    if (!check_refract(radius, center_host, n_inside, n_outside, fresnel, c, counts_out_host, s)) return bad_argument(nullptr);
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    if (ctx.empty()) return bad_argument(nullptr);
    return sum_shards(ctx, {{counts_out_host, 6}}, [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_refract_surface(one, radius, center_host, n_inside, n_outside, fresnel, c, seed, pass, p);
    });
}

struct gspectral_spec { // a call's arguments, checked; what the kernel reads
    int n_E = 0;
    double c[3] = {0.0, 0.0, 0.0};
    double R2 = 0.0, speed = 0.0;
    bool draws = false;         // some band has albedo < 1 or specular < 1: the ids are needed
    std::vector<double> tables; // albedo | specular | E edges
    size_t cells() const { return (size_t)4 + 2 * (size_t)n_E; }      // reflected, absorbed, mirrored, out of band | by band, twice
    size_t lds() const { return tables.size() * sizeof(double) + cells() * sizeof(uint32_t); }
    spans out(int64_t *counts, int64_t *bands) const { return {{counts, 4}, {bands, cells() - 4}}; }
};

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.
bool check_gspectral(double radius, const double *center, int n_E, const double *E_edges, const double *albedo, const double *specular,
                     double c, const int64_t *counts_out, const int64_t *bands_out, gspectral_spec &s) {
    if (!counts_out || !bands_out || !E_edges || !albedo || !specular || n_E < 1 || n_E > PCL_SPECTRAL_MAX_BANDS) return false;
    s.R2 = radius * radius;
    if (!std::isfinite(radius) || !(radius > 0) || !std::isfinite(s.R2) || !std::isfinite(c)) return false;
    if (center) {
        if (!finite3(center)) return false;
        for (int k = 0; k < 3; ++k) s.c[k] = center[k];
    }
    s.n_E = n_E; s.speed = c;
    for (const double *tab : {albedo, specular})
        for (int k = 0; k < n_E; ++k) {
            if (!(tab[k] >= 0.0 && tab[k] <= 1.0)) return false;        // (NaN as well)
            s.draws = s.draws || tab[k] < 1.0;                          // (specular < 1: somebody may leave by Lambert's block)
            s.tables.push_back(tab[k]);
        }
    return check_edges(E_edges, n_E, kEdgePlain, &s.tables);
}

template <typename T>
int launch_gspectral(pcl_ctx *ctx, const store_view &v, const gspectral_spec &s, uint64_t seed, uint32_t pass, const staged &st) {
    gspectral_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *vel = nullptr, *dr = nullptr, *dv = nullptr;
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &vel));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DR0 + k, &dr));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DV0 + k, &dv));
        a.r[k] = static_cast<T *>(r); a.v[k] = static_cast<T *>(vel);
        a.dr[k] = static_cast<T *>(dr); a.dv[k] = static_cast<T *>(dv);
        a.c[k] = s.c[k];
    }
    // E is always asked for (the band is the point of the call): the pointer costs a wavelength-dependent scatter step its term
    // cache (pcl_shell.hip), every pass.
    void *E = nullptr;
    PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_E, &E));
    a.E = static_cast<const T *>(E); a.kind = st.kind; a.ids = st.ids; a.tables = st.tables; a.out = st.out;
    a.N = v.N; a.ts = v.ts; a.id_base = st.id_base; a.tile_log = v.tile_log; a.n_E = s.n_E;
    a.R2 = s.R2; a.speed = s.speed;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.pass = pass;
    const size_t lds = s.lds();                                         // 56 B for one band, 32 KiB for 1024
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(lds));
    hipLaunchKernelGGL(k_ground_spectral<T>, dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int ground_spectral(pcl_ctx *ctx, double radius, const double *center_host, int n_bands, const double *E_edges_host,
                    const double *albedo_host, const double *specular_host, double c, uint64_t seed, uint32_t pass,
                    int64_t *counts_out_host, int64_t *bands_out_host) {
    gspectral_spec s;
    if (!ctx || !check_gspectral(radius, center_host, n_bands, E_edges_host, albedo_host, specular_host, c, counts_out_host, bands_out_host, s))
        return bad_argument(ctx);
    const spans out = s.out(counts_out_host, bands_out_host);
    store_view v;
    staged st(ctx);
    PCL_SWEEP_TRY(open_store(ctx, PCL_R0, &v));
    zero_spans(out);
    if (v.N <= 0) return PCL_OK;
    PCL_SWEEP_TRY(stage(st, v, s.cells(), s.tables.data(), s.tables.size(), s.draws));   // the ids only if somebody may draw
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_gspectral, ctx, v, s, seed, pass, st));
    return fetch(st, out);
}

int group_ground_spectral(pcl_group *group, double radius, const double *center_host, int n_bands, const double *E_edges_host,
                          const double *albedo_host, const double *specular_host, double c, uint64_t seed, uint32_t pass,
                          int64_t *counts_out_host, int64_t *bands_out_host) {
    gspectral_spec s;                                                   // the arguments first: a refused call looks at no group
    if (!check_gspectral(radius, center_host, n_bands, E_edges_host, albedo_host, specular_host, c, counts_out_host, bands_out_host, s))
        return bad_argument(nullptr);
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    if (ctx.empty()) return bad_argument(nullptr);
    return sum_shards(ctx, s.out(counts_out_host, bands_out_host), [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_ground_spectral(one, radius, center_host, n_bands, E_edges_host, albedo_host, specular_host, c, seed, pass, p, p + 4);
    });
}

// ---- scattering by layer and band: the kernel stands with its host side, behind the older sweeps (their tests read the file by its order)
// The counter words of a scattering by layer and band: who scatters, where to (the header lists who uses which word: 23 and 24
// are this kernel's alone).
constexpr uint32_t kLayeredScatterDraw = 23, kLayeredScatterDir = 24;

template <typename T>
struct lscatter_args {
    const T *r[3];               // read only with layers
    T *v[3], *dv[3];
    const T *E;                  // NULL without energy bands
    const unsigned char *kind;   // NULL: every particle is a photon
    const int64_t *ids;          // NULL: the id of slot i is id_base + i
    const double *tables;        // p (L' x B') | e*e of the layer edges (L + 1, if L) | E edges (B + 1, if B), device
    unsigned long long *out;     // exposed, scattered | scattered by cell [L' x B']; device, zeroed by the entry point
    int64_t N, ts, id_base;      // particles, tile stride of the slab (elements), id of slot 0
    int tile_log;                // log2 of the tile length
    int n_layers, n_E;           // L (0: one row of p everywhere, L' = 1), B (0: one column for every energy, B' = 1)
    int first;                   // 1: the pass's first scatterer -- a photon that is not scattered gets dv = 0
    double c[3], speed;
    uint32_t k0, k1, pass;       // Philox key (seed_lo, seed_hi), the step's own pass counter
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_scatter_layered(lscatter_args<T> a) {
    extern __shared__ double s_mem[];                                  // p | e*e | E edges | exposed, scattered | by cell
    const int L = a.n_layers, Lp = L > 0 ? L : 1, nE = a.n_E, Bp = nE > 0 ? nE : 1;
    const int n_tab = Lp * Bp + (L ? L + 1 : 0) + (nE ? nE + 1 : 0);
    const int n_cells = 2 + Lp * Bp;
    const double *s_p = s_mem;
    const double *s_e2 = s_p + Lp * Bp;
    const double *s_E = s_e2 + (L ? L + 1 : 0);
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_mem + n_tab);
    uint32_t *s_cell = s_cnt + 2;
    for (int k = threadIdx.x; k < n_tab; k += kBlock) s_mem[k] = a.tables[k];
    for (int k = threadIdx.x; k < n_cells; k += kBlock) s_cnt[k] = 0;  // (the cells follow the two counts)
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = grid_stride(), n_round = whole_waves(a.N);   // (the ballots below need whole waves inside the loop)
    for (int64_t i = first_slot(); i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        bool photon = in;
        if (photon && a.kind) photon = a.kind[i] != 0;                  // plain Objects are never touched
        // moving: at_rest, written out as in k_absorb_path and negated -- -0.0 == 0, a NaN moves, v0 != 0 loads no more of v
        const bool go = photon && !((double)a.v[0][ti] == 0.0 && (double)a.v[1][ti] == 0.0 && (double)a.v[2][ti] == 0.0);
        int b = go && L == 0 ? 0 : -1;                                  // the layer; -1: in no layer
        if (go && L > 0) {
            double x[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = __dsub_rn((double)a.r[k][ti], a.c[k]);   // fp32 widens exactly
            const double q = dot3(x, x);
            if (q >= s_e2[0] && q <= s_e2[L]) b = bin_of(s_e2, L, q);   // (dist2, closed_bin: written out) NaN: in no layer
        }
        int cell = b >= 0 && nE == 0 ? b : -1;                          // b * B' + e; -1: not exposed
        if (b >= 0 && nE > 0) {
            const double e = (double)a.E[ti];
            if (e >= s_E[0] && e <= s_E[nE]) cell = b * nE + bin_of(s_E, nE, e);         // NaN and under/overflow: in no band
        }
        const bool exposed = cell >= 0;
        bool hit = false;
        uint64_t id = 0;
        if (exposed) {
            const double p = s_p[cell];
            if (p > 0.0) {                                              // a clear cell draws nothing
                id = id_of(a.ids, a.id_base, i);
                hit = first_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kLayeredScatterDraw, a.k0, a.k1)) < p;   // u < 1: p == 1 scatters everybody
            }
        }
        const uint32_t n_exp = (uint32_t)__popcll(__ballot(exposed)), n_hit = (uint32_t)__popcll(__ballot(hit));
        if (lane == 0 && n_exp) atomicAdd(&s_cnt[0], n_exp);
        if (lane == 0 && n_hit) atomicAdd(&s_cnt[1], n_hit);
        if (a.first && photon && !hit) {                                // the scatter step's miss: "did not scatter", the three rows together
#pragma unroll
            for (int k = 0; k < 3; ++k) a.dv[k][ti] = (T)0.0;
        }
        if (!hit) continue;     // lanes that are left alone wait at the loop's head: no ballot below this line
        atomicAdd(&s_cell[cell], 1u);
        double u_a, u_b, sc, ss, e1[3], e2[3];
        const double w[3] = {1.0, 0.0, 0.0};
        pair_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kLayeredScatterDir, a.k0, a.k1), &u_a, &u_b);
        const double mu = __dsub_rn(1.0, __dmul_rn(2.0, u_a));                                       // uniform on the sphere
        polar(mu, u_b, &sc, &ss);
        frame(w, e1, e2);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double vo = (double)a.v[k][ti];                       // the velocity before the scatter (fp32 widens exactly)
            const double vk = __dmul_rn(a.speed, turned(sc, ss, mu, e1[k], e2[k], w[k]));
            a.v[k][ti] = (T)vk;
            a.dv[k][ti] = (T)__dsub_rn(vk, vo);
        }
    }
    __syncthreads();
    // pcl_sweep::flush_cells, written out, for the reason given in k_absorb_scattered: a further caller changes the older kernels
    for (int k = threadIdx.x; k < n_cells; k += kBlock)
        if (s_cnt[k]) atomicAdd(&a.out[k], (unsigned long long)s_cnt[k]);
}

// The scattering by layer and band takes pcl_step_absorb_path's tables by pcl_step_absorb_path's check: the limits are the same.
static_assert(PCL_SCATTER_LAYERED_MAX_LAYERS == PCL_PATH_ABSORB_MAX_LAYERS && PCL_SCATTER_LAYERED_MAX_BANDS == PCL_PATH_ABSORB_MAX_BANDS &&
              PCL_SCATTER_LAYERED_MAX_CELLS == PCL_PATH_ABSORB_MAX_CELLS, "one check serves both sweeps");

struct lscatter_spec { // a call's arguments, checked; what the kernel compares against
    pabsorb_spec tab;           // p | e*e | E edges, the centre, who draws: cells() = exposed, scattered | by cell
    int first = 0;
    double speed = 0.0;
};

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.
bool check_lscatter(int n_layers, int n_E, const double *p, const double *edges, const double *center, const double *E_edges, int first,
                    double c, const int64_t *counts_out, const int64_t *cells_out, lscatter_spec &s) {
    if ((first != 0 && first != 1) || !std::isfinite(c)) return false;
    s.first = first; s.speed = c;
    return check_pabsorb(n_layers, n_E, p, edges, center, E_edges, counts_out, cells_out, s.tab);
}

template <typename T>
int launch_lscatter(pcl_ctx *ctx, const store_view &v, const lscatter_spec &s, uint64_t seed, uint32_t pass, const staged &st) {
    lscatter_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *vel = nullptr, *dv = nullptr;
        if (s.tab.n_layers > 0) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &vel));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DV0 + k, &dv));     // (what makes a lazy dv real: a hit's and, with first, a miss's is written)
        a.r[k] = static_cast<const T *>(r); a.v[k] = static_cast<T *>(vel); a.dv[k] = static_cast<T *>(dv);
        a.c[k] = s.tab.c[k];
    }
    // E is asked for only with energy bands: the pointer costs a wavelength-dependent scatter step its term cache (pcl_shell.hip).
    void *E = nullptr;
    if (s.tab.n_E > 0) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_E, &E));
    a.E = static_cast<const T *>(E); a.kind = st.kind; a.ids = st.ids; a.tables = st.tables; a.out = st.out;
    a.N = v.N; a.ts = v.ts; a.id_base = st.id_base; a.tile_log = v.tile_log;
    a.n_layers = s.tab.n_layers; a.n_E = s.tab.n_E; a.first = s.first; a.speed = s.speed;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.pass = pass;
    const size_t lds = s.tab.lds();                                     // what this call uses: 24 B for one cell everywhere
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(lds));
    hipLaunchKernelGGL(k_scatter_layered<T>, dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int scatter_layered(pcl_ctx *ctx, int n_layers, int n_E_bins, const double *p_host, const double *edges_host, const double *center_host,
                    const double *E_edges_host, int first, double c, uint64_t seed, uint32_t pass, int64_t *counts_out_host,
                    int64_t *cells_out_host) {
    lscatter_spec s;
    if (!ctx || !check_lscatter(n_layers, n_E_bins, p_host, edges_host, center_host, E_edges_host, first, c, counts_out_host, cells_out_host, s))
        return bad_argument(ctx);
    const spans out = s.tab.out(counts_out_host, cells_out_host);
    store_view v;
    staged st(ctx);
    PCL_SWEEP_TRY(open_store(ctx, PCL_V0, &v));
    zero_spans(out);
    if (v.N <= 0) return PCL_OK;
    PCL_SWEEP_TRY(stage(st, v, s.tab.cells(), s.tab.tables.data(), s.tab.tables.size(), s.tab.draws));   // the ids only if somebody may draw
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_lscatter, ctx, v, s, seed, pass, st));
    return fetch(st, out);
}

int group_scatter_layered(pcl_group *group, int n_layers, int n_E_bins, const double *p_host, const double *edges_host,
                          const double *center_host, const double *E_edges_host, int first, double c, uint64_t seed, uint32_t pass,
                          int64_t *counts_out_host, int64_t *cells_out_host) {
    lscatter_spec s;                                                    // the arguments first: a refused call looks at no group
    if (!check_lscatter(n_layers, n_E_bins, p_host, edges_host, center_host, E_edges_host, first, c, counts_out_host, cells_out_host, s))
        return bad_argument(nullptr);
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    if (ctx.empty()) return bad_argument(nullptr);
    return sum_shards(ctx, s.tab.out(counts_out_host, cells_out_host), [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_scatter_layered(one, n_layers, n_E_bins, p_host, edges_host, center_host, E_edges_host, first, c, seed, pass, p, p + 2);
    });
}

// ---- scattering on a grid of cells: the kernel stands with its host side, behind the older sweeps (their tests read the file by its order)
// The counter words of a scattering on a grid: who scatters, where to (the header lists who uses which word: 25 and 26 are this
// kernel's alone).
constexpr uint32_t kGridScatterDraw = 25, kGridScatterDir = 26;
// The LDS form's switch-over: up to this many cells the probabilities and a workgroup's tallies sit in LDS beside the edges, if
// the whole stays within what a launch may ask for; above it both stay in device memory.
constexpr int kGridScatterLdsCells = 4096;
constexpr size_t kGridScatterLdsBytes = 64 * 1024;
static_assert(PCL_SCATTER_GRID_MAX_CELLS == PCL_GRID_MAX_CELLS, "the medium's grid is the position grid's");

template <typename T>
struct gscatter_args {
    const T *r[3];               // rows some axis needs (NULL otherwise)
    T *v[3], *dv[3];
    const T *E;                  // NULL without energy bands
    const unsigned char *kind;   // NULL: every particle is a photon
    const int64_t *ids;          // NULL: the id of slot i is id_base + i
    const double *tables;        // p [n_cells] | the axes' edges one after another (a radius axis: squared) | E edges (B + 1, if B), device
    unsigned long long *out;     // exposed, scattered | scattered by cell [n_cells]; device, zeroed by the entry point
    int64_t N, ts, id_base;      // particles, tile stride of the slab (elements), id of slot 0
    int tile_log;                // log2 of the tile length
    int n_axes, n_E;             // axes of the grid, B (0: one column for every energy, B' = 1)
    int n_edges, n_cells;        // every edge of the axes and of E; cells of the grid x B'
    int coord[PCL_GRID_MAX_AXES], n_bins[PCL_GRID_MAX_AXES], edge_at[PCL_GRID_MAX_AXES], E_at;
    int rows;                    // bit k: row k of r is read
    int first;                   // 1: the pass's first scatterer -- a photon that is not scattered gets dv = 0
    double c[3], speed;
    uint32_t k0, k1, pass;       // Philox key (seed_lo, seed_hi), the step's own pass counter
};

template <typename T, bool kLds>
__global__ void __launch_bounds__(kBlock) k_scatter_grid(gscatter_args<T> a) {
    extern __shared__ double s_mem[];                                  // edges | p (LDS form) | exposed, scattered | by cell (LDS form)
    const int nE = a.n_E, n_lds_p = kLds ? a.n_cells : 0;
    double *s_edges = s_mem;
    double *s_p = s_mem + a.n_edges;
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_p + n_lds_p);
    uint32_t *s_cell = s_cnt + 2;
    const int n_cnt = 2 + n_lds_p;
    for (int k = threadIdx.x; k < a.n_edges; k += kBlock) s_edges[k] = a.tables[a.n_cells + k];
    for (int k = threadIdx.x; k < n_lds_p; k += kBlock) s_p[k] = a.tables[k];
    for (int k = threadIdx.x; k < n_cnt; k += kBlock) s_cnt[k] = 0;    // (the cells follow the two counts)
    __syncthreads();
    const double *s_E = s_edges + a.E_at;
    const int lane = threadIdx.x & 63;
    const int64_t stride = grid_stride(), n_round = whole_waves(a.N);   // (the ballots below need whole waves inside the loop)
    // wave-uniform, as in k_position_grid: the cell and the count of consecutive trips whose hit lanes all sat in that one cell,
    // not added yet (fewer than 2^32: kMaxSlotsPerWorkgroup).  Every bulk run starts with all photons in ONE cell, and adds to one
    // address serialise where they are carried out; so a run is added once.
    int run_cell = 0;
    uint32_t run_n = 0;
    auto flush_run = [&]() {
        if (lane == 0 && run_n) {
            if (kLds) atomicAdd(&s_cell[run_cell], run_n);
            else atomicAdd(&a.out[2 + run_cell], (unsigned long long)run_n);
        }
        run_n = 0;
    };
    for (int64_t i = first_slot(); i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        bool photon = in;
        if (photon && a.kind) photon = a.kind[i] != 0;                  // plain Objects are never touched
        // moving: at_rest, written out as in k_scatter_layered and negated -- -0.0 == 0, a NaN moves, v0 != 0 loads no more of v
        const bool go = photon && !((double)a.v[0][ti] == 0.0 && (double)a.v[1][ti] == 0.0 && (double)a.v[2][ti] == 0.0);
        int cell = -1;                                                  // (cell of the grid) * B' + e; -1: not exposed
        if (go) {
            double x[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if ((a.rows >> k) & 1) x[k] = (double)a.r[k][ti];       // fp32 widens exactly
            bool ok = true;
            int at = 0;
            for (int ax = 0; ax < a.n_axes; ++ax) {                     // k_position_grid's lines
                const int co = a.coord[ax], nb = a.n_bins[ax];
                const double *e = s_edges + a.edge_at[ax];
                double q;
                if (co == PCL_GRID_RADIUS) {   // q, unfused, in this order (the library is built with -ffp-contract=off)
                    const double dx = x[0] - a.c[0], dy = x[1] - a.c[1], dz = x[2] - a.c[2];
                    q = (dx * dx + dy * dy) + dz * dz;
                } else {
                    q = co == 0 ? x[0] : (co == 1 ? x[1] : x[2]);
                }
                ok = ok && q >= e[0] && q <= e[nb];                     // NaN and anything outside the axis's range are in no cell
                at = at * nb + bin_of(e, nb, q);
            }
            if (ok && nE > 0) {
                const double e = (double)a.E[ti];
                ok = e >= s_E[0] && e <= s_E[nE];                       // NaN and under/overflow: in no band
                at = at * nE + bin_of(s_E, nE, e);
            }
            if (ok) cell = at;
        }
        const bool exposed = cell >= 0;
        bool hit = false;
        uint64_t id = 0;
        if (exposed) {
            const double p = kLds ? s_p[cell] : a.tables[cell];         // (global form: a read-only load, the table stays in L2)
            if (p > 0.0) {                                              // a clear cell draws nothing
                id = id_of(a.ids, a.id_base, i);
                hit = first_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kGridScatterDraw, a.k0, a.k1)) < p;   // u < 1: p == 1 scatters everybody
            }
        }
        const unsigned long long m_hit = __ballot(hit);
        const uint32_t n_exp = (uint32_t)__popcll(__ballot(exposed)), n_hit = (uint32_t)__popcll(m_hit);
        if (lane == 0 && n_exp) atomicAdd(&s_cnt[0], n_exp);
        if (lane == 0 && n_hit) atomicAdd(&s_cnt[1], n_hit);
        bool counted = false;                                           // this lane's hit is in the wave's run
        if (m_hit) {                                                    // (wave-uniform)
            const int c0 = __shfl(cell, __ffsll((long long)m_hit) - 1);
            if (__ballot(hit && cell == c0) == m_hit) {                 // every hit lane of the wave in one cell: one add of their count,
                if (c0 != run_cell) {                                   // put off while the next trips hit in the same cell
                    flush_run();
                    run_cell = c0;
                }
                run_n += n_hit;
                counted = true;
            }
        }
        if (a.first && photon && !hit) {                                // the scatter step's miss: "did not scatter", the three rows together
#pragma unroll
            for (int k = 0; k < 3; ++k) a.dv[k][ti] = (T)0.0;
        }
        if (!hit) continue;     // lanes that are left alone wait at the loop's head: no ballot below this line
        if (!counted) {
            if (kLds) atomicAdd(&s_cell[cell], 1u);
            else atomicAdd(&a.out[2 + cell], 1ull);
        }
        double u_a, u_b, sc, ss, e1[3], e2[3];
        const double w[3] = {1.0, 0.0, 0.0};
        pair_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kGridScatterDir, a.k0, a.k1), &u_a, &u_b);
        const double mu = __dsub_rn(1.0, __dmul_rn(2.0, u_a));                                       // uniform on the sphere
        polar(mu, u_b, &sc, &ss);
        frame(w, e1, e2);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double vo = (double)a.v[k][ti];                       // the velocity before the scatter (fp32 widens exactly)
            const double vk = __dmul_rn(a.speed, turned(sc, ss, mu, e1[k], e2[k], w[k]));
            a.v[k][ti] = (T)vk;
            a.dv[k][ti] = (T)__dsub_rn(vk, vo);
        }
    }
    flush_run();
    __syncthreads();
    // pcl_sweep::flush_cells, written out, for the reason given in k_absorb_scattered: a further caller changes the older kernels
    for (int k = threadIdx.x; k < n_cnt; k += kBlock)
        if (s_cnt[k]) atomicAdd(&a.out[k], (unsigned long long)s_cnt[k]);
}

struct gscatter_spec { // a call's arguments, checked; what the kernel compares against
    int n_axes = 0, n_E = 0, n_edges = 0, rows = 0, E_at = 0;
    int64_t n_p = 1;            // cells of the grid x B'
    int coord[PCL_GRID_MAX_AXES], n_bins[PCL_GRID_MAX_AXES], edge_at[PCL_GRID_MAX_AXES];
    double c[3] = {0.0, 0.0, 0.0}, speed = 0.0;
    int first = 0;
    bool draws = false;         // some cell has p > 0: the ids are needed
    std::vector<double> tables; // p | the axes' edges (a radius axis: squared) | E edges
    size_t cells() const { return (size_t)2 + (size_t)n_p; }            // exposed, scattered | by cell
    size_t lds_small() const { return (size_t)n_edges * sizeof(double) + 2 * sizeof(uint32_t); }               // the global form's
    size_t lds_whole() const { return lds_small() + (size_t)n_p * (sizeof(double) + sizeof(uint32_t)); }       // the LDS form's
    bool lds_form() const { return n_p <= kGridScatterLdsCells && lds_whole() <= kGridScatterLdsBytes; }
    spans out(int64_t *counts, int64_t *by_cell) const { return {{counts, 2}, {by_cell, (size_t)n_p}}; }
};

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.  The geometry
// by pcl_grid.hip's check_spec, p by check_pabsorb, first and c by check_lscatter.
bool check_gscatter(int n_axes, const int *coords, const int *n_bins, const double *edges, const double *center, int n_E,
                    const double *E_edges, const double *p, int first, double c, const int64_t *counts_out, const int64_t *cells_out,
                    gscatter_spec &s) {
    if ((first != 0 && first != 1) || !std::isfinite(c)) return false;
    if (!coords || !n_bins || !edges || !p || !counts_out || !cells_out) return false;
    if (n_axes < 1 || n_axes > PCL_GRID_MAX_AXES || n_E < 0 || n_E > PCL_SCATTER_GRID_MAX_BANDS || (n_E > 0 && !E_edges)) return false;
    s.first = first; s.speed = c; s.n_axes = n_axes; s.n_E = n_E;
    int seen = 0;
    for (int a = 0; a < n_axes; ++a) {
        if (coords[a] < PCL_GRID_X || coords[a] > PCL_GRID_RADIUS || ((seen >> coords[a]) & 1)) return false;
        seen |= 1 << coords[a];
        if (n_bins[a] < 1 || n_bins[a] > PCL_GRID_MAX_BINS) return false;
        s.n_p *= n_bins[a];
    }
    s.n_p *= n_E > 0 ? n_E : 1;                                          // (below 2^41: no overflow)
    if (s.n_p > PCL_SCATTER_GRID_MAX_CELLS) return false;
    if (center)
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(center[k])) return false;
            s.c[k] = center[k];
        }
    s.tables.reserve((size_t)s.n_p + 4 * (PCL_GRID_MAX_BINS + 1));
    for (int64_t k = 0; k < s.n_p; ++k) {
        if (!(p[k] >= 0.0 && p[k] <= 1.0)) return false;                // (NaN as well)
        s.draws = s.draws || p[k] > 0.0;
        s.tables.push_back(p[k]);
    }
    for (int a = 0; a < n_axes; ++a) {
        s.coord[a] = coords[a];
        s.n_bins[a] = n_bins[a];
        s.edge_at[a] = s.n_edges;
        s.rows |= coords[a] == PCL_GRID_RADIUS ? 7 : 1 << coords[a];
        // q of a radius axis is compared against e*e: no square root anywhere
        if (!check_edges(edges + s.n_edges, n_bins[a], coords[a] == PCL_GRID_RADIUS ? kEdgeSquare : kEdgePlain, &s.tables)) return false;
        s.n_edges += n_bins[a] + 1;
    }
    s.E_at = s.n_edges;
    if (n_E > 0) {
        if (!check_edges(E_edges, n_E, kEdgePlain, &s.tables)) return false;
        s.n_edges += n_E + 1;
    }
    return true;
}

template <typename T>
int launch_gscatter(pcl_ctx *ctx, const store_view &v, const gscatter_spec &s, uint64_t seed, uint32_t pass, const staged &st) {
    gscatter_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *vel = nullptr, *dv = nullptr;
        if ((s.rows >> k) & 1) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &vel));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DV0 + k, &dv));     // (what makes a lazy dv real: a hit's and, with first, a miss's is written)
        a.r[k] = static_cast<const T *>(r); a.v[k] = static_cast<T *>(vel); a.dv[k] = static_cast<T *>(dv);
        a.c[k] = s.c[k];
    }
    // E is asked for only with energy bands: the pointer costs a wavelength-dependent scatter step its term cache (pcl_shell.hip).
    void *E = nullptr;
    if (s.n_E > 0) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_E, &E));
    a.E = static_cast<const T *>(E); a.kind = st.kind; a.ids = st.ids; a.tables = st.tables; a.out = st.out;
    a.N = v.N; a.ts = v.ts; a.id_base = st.id_base; a.tile_log = v.tile_log;
    a.n_axes = s.n_axes; a.n_E = s.n_E; a.n_edges = s.n_edges; a.n_cells = (int)s.n_p; a.E_at = s.E_at; a.rows = s.rows;
    for (int k = 0; k < s.n_axes; ++k) { a.coord[k] = s.coord[k]; a.n_bins[k] = s.n_bins[k]; a.edge_at[k] = s.edge_at[k]; }
    a.first = s.first; a.speed = s.speed;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.pass = pass;
    const bool lds_form = s.lds_form();
    const size_t lds = lds_form ? s.lds_whole() : s.lds_small();
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(lds));
    if (lds_form) hipLaunchKernelGGL((k_scatter_grid<T, true>), dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    else hipLaunchKernelGGL((k_scatter_grid<T, false>), dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int scatter_grid(pcl_ctx *ctx, int n_axes, const int *coords_host, const int *n_bins_host, const double *edges_host,
                 const double *center_host, int n_E_bins, const double *E_edges_host, const double *p_host, int first, double c,
                 uint64_t seed, uint32_t pass, int64_t *counts_out_host, int64_t *cells_out_host) {
    gscatter_spec s;
    if (!ctx || !check_gscatter(n_axes, coords_host, n_bins_host, edges_host, center_host, n_E_bins, E_edges_host, p_host, first, c,
                                counts_out_host, cells_out_host, s))
        return bad_argument(ctx);
    const spans out = s.out(counts_out_host, cells_out_host);
    store_view v;
    staged st(ctx);
    PCL_SWEEP_TRY(open_store(ctx, PCL_V0, &v));
    zero_spans(out);
    if (v.N <= 0) return PCL_OK;
    PCL_SWEEP_TRY(stage(st, v, s.cells(), s.tables.data(), s.tables.size(), s.draws));   // the ids only if somebody may draw
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_gscatter, ctx, v, s, seed, pass, st));
    return fetch(st, out);
}

int group_scatter_grid(pcl_group *group, int n_axes, const int *coords_host, const int *n_bins_host, const double *edges_host,
                       const double *center_host, int n_E_bins, const double *E_edges_host, const double *p_host, int first, double c,
                       uint64_t seed, uint32_t pass, int64_t *counts_out_host, int64_t *cells_out_host) {
    gscatter_spec s;                                                    // the arguments first: a refused call looks at no group
    if (!check_gscatter(n_axes, coords_host, n_bins_host, edges_host, center_host, n_E_bins, E_edges_host, p_host, first, c,
                        counts_out_host, cells_out_host, s))
        return bad_argument(nullptr);
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    if (ctx.empty()) return bad_argument(nullptr);
    return sum_shards(ctx, s.out(counts_out_host, cells_out_host), [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_scatter_grid(one, n_axes, coords_host, n_bins_host, edges_host, center_host, n_E_bins, E_edges_host, p_host, first,
                                     c, seed, pass, p, p + 2);
    });
}

// ---- box walls: the kernel stands with its host side, at the end of the unit, as the scattering on a grid does
template <typename T>
struct walls_args {
    T *r[3];                     // the axes with a wall (NULL otherwise)
    T *v[3];                     // always: who moves
    T *dr[3];                    // the mirror axes (NULL otherwise)
    T *dv[3];                    // the mirror axes, and all three with an open wall (NULL otherwise)
    const unsigned char *kind;   // NULL: every particle is a photon
    unsigned long long *out;     // [8]: moving, multi, crossed[3][2]; device, zeroed by the entry point
    int64_t N, ts;               // particles, tile stride of the slab (elements)
    int tile_log;                // log2 of the tile length
    int mode[3];                 // PCL_WALL_* per axis
    double lo[3], hi[3], L[3];   // L = hi - lo, made on the host, once
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_box_walls(walls_args<T> a) {
    __shared__ uint32_t s_cnt[8];                                       // moving, multi, crossed[3][2]
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = grid_stride(), n_round = whole_waves(a.N);   // (the ballots below need whole waves inside the loop)
    for (int64_t i = first_slot(); i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        // moving: at_rest, written out as in k_absorb_path and negated -- -0.0 == 0, a NaN moves, v0 != 0 loads no more of v
        bool go = in && !((double)a.v[0][ti] == 0.0 && (double)a.v[1][ti] == 0.0 && (double)a.v[2][ti] == 0.0);
        if (go && a.kind) go = a.kind[i] != 0;                          // plain Objects are never touched
        int side[3] = {-1, -1, -1};                                     // 0 below, 1 above; -1: inside, no wall, or not finite
        double x[3] = {0.0, 0.0, 0.0};
        bool park = false;
        if (go) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (a.mode[k] != PCL_WALL_NONE) {
                    x[k] = (double)a.r[k][ti];                          // fp32 widens exactly
                    const bool below = x[k] < a.lo[k];
                    const bool above = a.mode[k] == PCL_WALL_PERIODIC ? x[k] >= a.hi[k] : x[k] > a.hi[k];   // (mirror, open: on the wall is inside)
                    if ((below || above) && x[k] > -INFINITY && x[k] < INFINITY) side[k] = below ? 0 : 1;   // NaN, +-inf: skipped
                    park = park || (side[k] >= 0 && a.mode[k] == PCL_WALL_OPEN);
                }
        }
        // the cell each axis counts in: with an open wall crossed only the first such axis, otherwise every axis that is outside
        int cell[3];
        bool seen = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool open_k = side[k] >= 0 && a.mode[k] == PCL_WALL_OPEN;
            cell[k] = park ? (open_k && !seen ? side[k] : -1) : side[k];
            seen = seen || open_k;
        }
        const bool fold = !park && (side[0] >= 0 || side[1] >= 0 || side[2] >= 0);
        double n[3] = {0.0, 0.0, 0.0}, f[3] = {0.0, 0.0, 0.0};
        bool multi = false;
        if (fold) {             // (no ballot inside: the lanes meet again behind this block)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (side[k] >= 0) {
                    const double s = __dsub_rn(x[k], a.lo[k]);
                    n[k] = floor(__ddiv_rn(s, a.L[k]));
                    f[k] = fmin(fmax(__dsub_rn(s, __dmul_rn(n[k], a.L[k])), 0.0), a.L[k]);
                    multi = multi || n[k] < -1.0 || n[k] > 1.0;
                }
        }
        const bool work = park || fold;
        const uint32_t n_go = (uint32_t)__popcll(__ballot(go));
        if (lane == 0 && n_go) atomicAdd(&s_cnt[0], n_go);
        if (__ballot(work)) {   // (the same answer in every lane of the wave)
            const uint32_t n_multi = (uint32_t)__popcll(__ballot(multi));
            if (lane == 0 && n_multi) atomicAdd(&s_cnt[1], n_multi);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint32_t n_lo = (uint32_t)__popcll(__ballot(cell[k] == 0)), n_hi = (uint32_t)__popcll(__ballot(cell[k] == 1));
                if (lane == 0 && n_lo) atomicAdd(&s_cnt[2 + 2 * k], n_lo);
                if (lane == 0 && n_hi) atomicAdd(&s_cnt[3 + 2 * k], n_hi);
            }
        }
        if (!work) continue;    // lanes that are left alone wait at the loop's head: no ballot below this line
        if (park) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {                               // park, written out: at rest where it is; r and dr stay
                a.v[k][ti] = (T)0.0;
                a.dv[k][ti] = (T)0.0;
            }
            continue;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (side[k] < 0) continue;
            if (a.mode[k] == PCL_WALL_PERIODIC) {
                double y = __dadd_rn(a.lo[k], f[k]);
                if (!(y < a.hi[k])) y = a.lo[k];
                a.r[k][ti] = (T)y;                                      // dr, v and dv stay: r - dr is the image of where it came from
            } else {
                const double h = __dmul_rn(n[k], 0.5);
                const bool odd = floor(h) != h;
                const double y = odd ? __dsub_rn(a.hi[k], f[k]) : __dadd_rn(a.lo[k], f[k]);
                a.r[k][ti] = (T)fmin(fmax(y, a.lo[k]), a.hi[k]);
                if (odd) {                                              // an odd number of bounces: the axis is turned round (a negation is exact)
                    a.v[k][ti] = -a.v[k][ti];
                    a.dv[k][ti] = -a.dv[k][ti];
                    a.dr[k][ti] = -a.dr[k][ti];
                }
            }
        }
    }
    __syncthreads();
    // pcl_sweep::flush_cells, written out, for the reason given in k_absorb_scattered: a further caller changes the older kernels
    for (int k = threadIdx.x; k < 8; k += kBlock)
        if (s_cnt[k]) atomicAdd(&a.out[k], (unsigned long long)s_cnt[k]);
}

struct walls_spec { // a call's arguments, checked; L is made here, once
    int mode[3] = {PCL_WALL_NONE, PCL_WALL_NONE, PCL_WALL_NONE};
    double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0}, L[3] = {1.0, 1.0, 1.0};
    bool open = false;          // some axis has an open wall: the three dv rows are written
};

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.
bool check_walls(const int *modes, const double *lo, const double *hi, const int64_t *counts_out, walls_spec &s) {
    if (!modes || !lo || !hi || !counts_out) return false;
    bool any = false;
    for (int k = 0; k < 3; ++k)
        if (modes[k] < PCL_WALL_NONE || modes[k] > PCL_WALL_OPEN) return false;
    for (int k = 0; k < 3; ++k) {
        s.mode[k] = modes[k];
        if (modes[k] == PCL_WALL_NONE) continue;                        // the bounds of an axis without a wall are not read
        const double L = hi[k] - lo[k];                                 // one rounding
        if (!std::isfinite(lo[k]) || !std::isfinite(hi[k]) || !std::isfinite(L) || !(L > 0)) return false;
        s.lo[k] = lo[k]; s.hi[k] = hi[k]; s.L[k] = L;
        s.open = s.open || modes[k] == PCL_WALL_OPEN;
        any = true;
    }
    return any;
}

template <typename T>
int launch_walls(pcl_ctx *ctx, const store_view &v, const walls_spec &s, const staged &st) {
    walls_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *vel = nullptr, *dr = nullptr, *dv = nullptr;
        const bool mirror = s.mode[k] == PCL_WALL_MIRROR;
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &vel));
        if (s.mode[k] != PCL_WALL_NONE) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        if (mirror) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DR0 + k, &dr));
        if (mirror || s.open) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DV0 + k, &dv));
        a.r[k] = static_cast<T *>(r); a.v[k] = static_cast<T *>(vel);
        a.dr[k] = static_cast<T *>(dr); a.dv[k] = static_cast<T *>(dv);
        a.mode[k] = s.mode[k]; a.lo[k] = s.lo[k]; a.hi[k] = s.hi[k]; a.L[k] = s.L[k];
    }
    a.kind = st.kind; a.out = st.out;
    a.N = v.N; a.ts = v.ts; a.tile_log = v.tile_log;
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(8 * sizeof(uint32_t)));
    hipLaunchKernelGGL(k_box_walls<T>, dim3((unsigned)grid), dim3(kBlock), 0, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int box_walls(pcl_ctx *ctx, const int *modes_host, const double *lo_host, const double *hi_host, int64_t *counts_out_host) {
    walls_spec s;
    if (!ctx || !check_walls(modes_host, lo_host, hi_host, counts_out_host, s)) return bad_argument(ctx);
    const spans out = {{counts_out_host, 8}};
    store_view v;                                                       // E is never asked for, ids never travel
    staged st(ctx);
    PCL_SWEEP_TRY(open_store(ctx, PCL_V0, &v));
    zero_spans(out);
    if (v.N <= 0) return PCL_OK;
    PCL_SWEEP_TRY(stage(st, v, 8, nullptr, 0, false));
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_walls, ctx, v, s, st));
    return fetch(st, out);
}

int group_box_walls(pcl_group *group, const int *modes_host, const double *lo_host, const double *hi_host, int64_t *counts_out_host) {
    walls_spec s;                                                       // the arguments first: a refused call looks at no group
    if (!check_walls(modes_host, lo_host, hi_host, counts_out_host, s)) return bad_argument(nullptr);
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    if (ctx.empty()) return bad_argument(nullptr);
    return sum_shards(ctx, {{counts_out_host, 8}}, [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_box_walls(one, modes_host, lo_host, hi_host, p);
    });
}

// ---- phase functions by grid cell: the kernel stands with its host side, at the end of the unit, as the scattering on a grid does
// What a launch may ask for of LDS: the tables, the edges and the cells of a call stay within it (the header states the bound).
constexpr size_t kGridPhaseLdsBytes = PCL_PHASE_GRID_LDS_BYTES;
constexpr unsigned kGridPhaseAlone = PCL_PHASE_GRID_ALONE;              // a cell's byte of the map: left alone
static_assert(PCL_PHASE_GRID_MAX_MIXTURES < PCL_PHASE_GRID_ALONE && PCL_PHASE_GRID_ALONE <= 255, "a mixture and the mark fit one byte of the map");
static_assert(PCL_PHASE_GRID_MAX_CELLS == PCL_GRID_MAX_CELLS, "the mixtures' grid is the position grid's");

template <typename T>
struct gphase_args {
    const T *r[3];               // rows some axis needs (NULL otherwise)
    T *v[3], *dv[3];
    const unsigned char *kind;   // NULL: every particle is a photon
    const int64_t *ids;          // NULL: the id of slot i is id_base + i
    const double *tables;        // C (K x M) | the axes' edges one after another (a radius axis: squared) | g (M) | mu, F, s (n_nodes each) | the laws' ints
    const unsigned char *map;    // one byte per cell of the grid: its row of C, kGridPhaseAlone: left alone; device, read by scattered lanes only
    unsigned long long *out;     // scattered, re-directed | by mixture [K] | by law [M]; device, zeroed by the entry point
    int64_t N, ts, id_base;      // particles, tile stride of the slab (elements), id of slot 0
    int tile_log;                // log2 of the tile length
    int n_mix, n_laws;           // K, M
    int n_nodes;                 // the nodes of all tables, bins + 1 each (0 without a table)
    int n_axes, n_edges;         // axes of the grid, every edge of the axes
    int coord[PCL_GRID_MAX_AXES], n_bins[PCL_GRID_MAX_AXES], edge_at[PCL_GRID_MAX_AXES];
    int rows;                    // bit k: row k of r is read
    int outside;                 // the row of C of a scattered photon in no cell; -1: left alone
    double c[3], speed;
    uint32_t k0, k1, pass;       // Philox key (seed_lo, seed_hi), the step's own pass counter
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_phase_grid(gphase_args<T> a) {
    extern __shared__ double s_mem[];                                  // tables | scattered, re-directed | by mixture | by law
    const int K = a.n_mix, M = a.n_laws, Tn = a.n_nodes;
    const int n_dbl = K * M + a.n_edges + M + 3 * Tn;
    const int n_tab = n_dbl + (3 * M + 1) / 2;                         // three ints per law, packed behind the doubles
    const int n_cells = 2 + K + M;
    const double *s_C = s_mem;
    const double *s_edges = s_C + K * M;
    const double *s_g = s_edges + a.n_edges;
    const double *s_mu = s_g + M;
    const double *s_F = s_mu + Tn;
    const double *s_s = s_F + Tn;
    const int *s_kind = reinterpret_cast<const int *>(s_mem + n_dbl);  // PCL_PHASE_* of law j
    const int *s_off = s_kind + M;                                     // a table's first node in mu, F and s
    const int *s_K = s_off + M;                                        // a table's bins
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_mem + n_tab);
    uint32_t *s_mix = s_cnt + 2;
    uint32_t *s_law = s_mix + K;
    for (int k = threadIdx.x; k < n_tab; k += kBlock) s_mem[k] = a.tables[k];
    for (int k = threadIdx.x; k < n_cells; k += kBlock) s_cnt[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = grid_stride(), n_round = whole_waves(a.N);   // (the ballots below need whole waves inside the loop)
    for (int64_t i = first_slot(); i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        double d[3] = {0.0, 0.0, 0.0}, o[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (in) d[k] = (double)a.dv[k][ti];                         // fp32 widens exactly
        // scattered in this pass: k_phase_layered's lines (scattered and workable)
        bool go = in && (d[0] != 0.0 || d[1] != 0.0 || d[2] != 0.0);
        if (go && a.kind) go = a.kind[i] != 0;
        if (go) {
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = __dsub_rn((double)a.v[k][ti], d[k]);      // the velocity before the scatter
        }
        const double oo = dot3(o, o);
        go = go && oo > 0.0 && oo < INFINITY;
        int b = -1;                                                     // the row of C; -1: left as the scatter step left it
        if (go) {
            double x[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if ((a.rows >> k) & 1) x[k] = (double)a.r[k][ti];       // fp32 widens exactly
            bool ok = true;
            int at = 0;
            for (int ax = 0; ax < a.n_axes; ++ax) {                     // k_position_grid's lines
                const int co = a.coord[ax], nb = a.n_bins[ax];
                const double *e = s_edges + a.edge_at[ax];
                double q;
                if (co == PCL_GRID_RADIUS) {   // q, unfused, in this order (the library is built with -ffp-contract=off)
                    const double dx = x[0] - a.c[0], dy = x[1] - a.c[1], dz = x[2] - a.c[2];
                    q = (dx * dx + dy * dy) + dz * dz;
                } else {
                    q = co == 0 ? x[0] : (co == 1 ? x[1] : x[2]);
                }
                ok = ok && q >= e[0] && q <= e[nb];                     // NaN and anything outside the axis's range are in no cell
                at = at * nb + bin_of(e, nb, q);
            }
            if (ok) {                                                   // (at is below the grid's cells: every bin is inside its axis)
                const unsigned m = a.map[at];                           // one byte, L2-resident over a sweep
                b = m == kGridPhaseAlone ? -1 : (int)m;
            } else {
                b = a.outside;
            }
        }
        const bool turn = b >= 0;
        const uint32_t n_go = (uint32_t)__popcll(__ballot(go)), n_turn = (uint32_t)__popcll(__ballot(turn));
        if (lane == 0 && n_go) atomicAdd(&s_cnt[0], n_go);
        if (lane == 0 && n_turn) {
            atomicAdd(&s_cnt[1], n_turn);
            if (K == 1) atomicAdd(&s_mix[0], n_turn);                   // one mixture, one law: the wave's count, not a lane's
            if (M == 1) atomicAdd(&s_law[0], n_turn);
        }
        if (!turn) continue;    // lanes that are left alone wait at the loop's head: no ballot below this line
        const uint64_t id = id_of(a.ids, a.id_base, i);
        int j = 0;
        if (M > 1) {
            const double *row = s_C + b * M;                            // cumulative, ends in 1: the first j with u_s < row[j]
            while (j < M - 1 && !(row[j] > 0.0)) ++j;                   // (u_s >= 0: a law without weight is never the first)
            if (row[j] < 1.0) {                                         // a one-hot row draws nothing
                const double u_s = first_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kLawWord, a.k0, a.k1));
                while (j < M - 1 && !(u_s < row[j])) ++j;
            }
            atomicAdd(&s_law[j], 1u);
        }
        if (K > 1) atomicAdd(&s_mix[b], 1u);
        const double on = __dsqrt_rn(oo);
        double w[3], sc, ss, e1[3], e2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = __ddiv_rn(o[k], on);
        double u_a, u_b;
        pair_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, 10u, a.k0, a.k1), &u_a, &u_b);
        const int law = s_kind[j];
        double mu = law_mu(law, s_g[j], u_a, id, a.pass, a.k0, a.k1);
        if (law == PCL_PHASE_TABLE) {                                   // the inverse of a piecewise linear F: 0 <= u_a < 1 is inside
            const int off = s_off[j];
            const int kb = off + bin_of(s_F + off, s_K[j], u_a);
            const double lo = s_mu[kb], hi = s_mu[kb + 1];
            mu = fmin(fmax(__dadd_rn(lo, __dmul_rn(__dsub_rn(u_a, s_F[kb]), s_s[kb])), lo), hi);
        }
        polar(mu, u_b, &sc, &ss);
        frame(w, e1, e2);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double vk = __dmul_rn(a.speed, turned(sc, ss, mu, e1[k], e2[k], w[k]));
            a.v[k][ti] = (T)vk;
            a.dv[k][ti] = (T)__dsub_rn(vk, o[k]);
        }
    }
    __syncthreads();
    // pcl_sweep::flush_cells, written out, for the reason given in k_absorb_scattered: a further caller changes the older kernels
    for (int k = threadIdx.x; k < n_cells; k += kBlock)
        if (s_cnt[k]) atomicAdd(&a.out[k], (unsigned long long)s_cnt[k]);
}

struct gphase_spec { // a call's arguments, checked; what the kernel reads
    lphase_spec laws;           // the laws and the rows of C by check_lphase (n_layers = 0: no edges of its own); its tables are taken over
    int n_mix = 0, n_axes = 0, n_edges = 0, rows = 0, outside = -1;
    int64_t n_grid = 1;         // cells of the grid
    int coord[PCL_GRID_MAX_AXES], n_bins[PCL_GRID_MAX_AXES], edge_at[PCL_GRID_MAX_AXES];
    std::vector<double> tables; // C | the axes' edges (a radius axis: squared) | g | mu | F | s | the laws' ints || the map, eight cells a double
    size_t n_lds = 0;           // the doubles in front of the map: what a workgroup copies into LDS
    size_t cells() const { return (size_t)2 + (size_t)n_mix + (size_t)laws.n_laws; }
    size_t lds() const { return n_lds * sizeof(double) + cells() * sizeof(uint32_t); }
};

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.  The laws by
// check_lphase (one row of C at a time), the geometry by check_gscatter's lines.
bool check_gphase(int n_laws, const int *kinds, const double *g, const int *law_bins, const double *mu, const double *F, int n_mix,
                  const double *cum, int n_axes, const int *coords, const int *n_bins, const double *edges, const double *center,
                  const unsigned char *map, int outside, double c, const int64_t *counts_out, gphase_spec &s) {
    if (!kinds || !cum || !coords || !n_bins || !edges || !map || !counts_out) return false;
    if (n_laws < 1 || n_laws > PCL_LPHASE_MAX_LAWS || n_mix < 1 || n_mix > PCL_PHASE_GRID_MAX_MIXTURES) return false;
    if (n_axes < 1 || n_axes > PCL_GRID_MAX_AXES || outside < -1 || outside >= n_mix) return false;
    const int M = n_laws;
    std::vector<double> rows_of_C;
    for (int m = 0; m < n_mix; ++m) {                                   // check_lphase takes one row without layers: K calls' rows, the last call's laws
        s.laws = lphase_spec();
        if (!check_lphase(n_laws, kinds, g, law_bins, mu, F, 0, cum + (size_t)m * M, nullptr, center, c, counts_out, s.laws)) return false;
        rows_of_C.insert(rows_of_C.end(), s.laws.tables.begin(), s.laws.tables.begin() + M);
    }
    s.n_mix = n_mix; s.n_axes = n_axes; s.outside = outside;
    int seen = 0;
    for (int a = 0; a < n_axes; ++a) {
        if (coords[a] < PCL_GRID_X || coords[a] > PCL_GRID_RADIUS || ((seen >> coords[a]) & 1)) return false;
        seen |= 1 << coords[a];
        if (n_bins[a] < 1 || n_bins[a] > PCL_GRID_MAX_BINS) return false;
        s.n_grid *= n_bins[a];
    }
    if (s.n_grid > PCL_PHASE_GRID_MAX_CELLS) return false;
    s.tables = rows_of_C;
    for (int a = 0; a < n_axes; ++a) {
        s.coord[a] = coords[a];
        s.n_bins[a] = n_bins[a];
        s.edge_at[a] = s.n_edges;
        s.rows |= coords[a] == PCL_GRID_RADIUS ? 7 : 1 << coords[a];
        // q of a radius axis is compared against e*e: no square root anywhere
        if (!check_edges(edges + s.n_edges, n_bins[a], coords[a] == PCL_GRID_RADIUS ? kEdgeSquare : kEdgePlain, &s.tables)) return false;
        s.n_edges += n_bins[a] + 1;
    }
    s.tables.insert(s.tables.end(), s.laws.tables.begin() + M, s.laws.tables.end());     // g | mu | F | s | the laws' ints
    s.n_lds = s.tables.size();
    if (s.lds() > kGridPhaseLdsBytes) return false;                     // the header's bound
    for (int64_t k = 0; k < s.n_grid; ++k)
        if (map[k] >= n_mix && map[k] != kGridPhaseAlone) return false;
    s.tables.resize(s.n_lds + ((size_t)s.n_grid + 7) / 8, 0.0);
    memcpy(s.tables.data() + s.n_lds, map, (size_t)s.n_grid);
    return true;
}

template <typename T>
int launch_gphase(pcl_ctx *ctx, const store_view &v, const gphase_spec &s, uint64_t seed, uint32_t pass, const staged &st) {
    gphase_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *vel = nullptr, *dv = nullptr;
        if ((s.rows >> k) & 1) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &vel));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DV0 + k, &dv));
        a.r[k] = static_cast<const T *>(r); a.v[k] = static_cast<T *>(vel); a.dv[k] = static_cast<T *>(dv);
        a.c[k] = s.laws.c[k];
    }
    a.kind = st.kind; a.ids = st.ids; a.tables = st.tables; a.out = st.out;
    a.map = reinterpret_cast<const unsigned char *>(st.tables + s.n_lds);
    a.N = v.N; a.ts = v.ts; a.id_base = st.id_base; a.tile_log = v.tile_log;
    a.n_mix = s.n_mix; a.n_laws = s.laws.n_laws; a.n_nodes = s.laws.n_nodes; a.n_axes = s.n_axes; a.n_edges = s.n_edges;
    for (int k = 0; k < s.n_axes; ++k) { a.coord[k] = s.coord[k]; a.n_bins[k] = s.n_bins[k]; a.edge_at[k] = s.edge_at[k]; }
    a.rows = s.rows; a.outside = s.outside; a.speed = s.laws.speed;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.pass = pass;
    const size_t lds = s.lds();                                         // what this call uses
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(lds));
    hipLaunchKernelGGL(k_phase_grid<T>, dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int phase_grid(pcl_ctx *ctx, int n_laws, const int *kinds, const double *g, const int *law_bins, const double *mu, const double *F,
               int n_mix, const double *cum, int n_axes, const int *coords, const int *n_bins, const double *edges, const double *center,
               const unsigned char *map, int outside, double c, uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    gphase_spec s;
    if (!ctx || !check_gphase(n_laws, kinds, g, law_bins, mu, F, n_mix, cum, n_axes, coords, n_bins, edges, center, map, outside, c,
                              counts_out_host, s))
        return bad_argument(ctx);
    const spans out = {{counts_out_host, s.cells()}};
    store_view v;                                                       // E is never asked for, as in phase_layered
    staged st(ctx);
    PCL_SWEEP_TRY(open_store(ctx, PCL_DV0, &v));
    zero_spans(out);
    if (v.N <= 0) return PCL_OK;
    PCL_SWEEP_TRY(stage(st, v, s.cells(), s.tables.data(), s.tables.size(), true));
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_gphase, ctx, v, s, seed, pass, st));
    return fetch(st, out);
}

int group_phase_grid(pcl_group *group, int n_laws, const int *kinds, const double *g, const int *law_bins, const double *mu,
                     const double *F, int n_mix, const double *cum, int n_axes, const int *coords, const int *n_bins, const double *edges,
                     const double *center, const unsigned char *map, int outside, double c, uint64_t seed, uint32_t pass,
                     int64_t *counts_out_host) {
    gphase_spec s;                                                      // the arguments first: a refused call looks at no group
    if (!check_gphase(n_laws, kinds, g, law_bins, mu, F, n_mix, cum, n_axes, coords, n_bins, edges, center, map, outside, c,
                      counts_out_host, s))
        return bad_argument(nullptr);
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    if (ctx.empty()) return bad_argument(nullptr);
    return sum_shards(ctx, {{counts_out_host, s.cells()}}, [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_phase_grid(one, n_laws, kinds, g, law_bins, mu, F, n_mix, cum, n_axes, coords, n_bins, edges, center, map, outside,
                                   c, seed, pass, p);
    });
}

// ---- absorption on a grid of cells: the kernel stands with its host side, at the end of the unit, as the scattering on a grid does
// The counter words of an absorption on a grid: along the path, at the interaction (the header lists who uses which word: 27 and 28
// are this kernel's alone).
constexpr uint32_t kGridAbsorbPath = 27, kGridAbsorbHit = 28;
// The LDS form's switch-over (the header states the formula): up to this many cells the tables given and a workgroup's tallies sit in
// LDS beside the edges, if the whole stays within what a launch may ask for; above it both stay in device memory.
constexpr int kGridAbsorbLdsCells = PCL_ABSORB_GRID_LDS_CELLS;
constexpr size_t kGridAbsorbLdsBytes = PCL_ABSORB_GRID_LDS_BYTES;
static_assert(PCL_ABSORB_GRID_MAX_CELLS == PCL_GRID_MAX_CELLS && PCL_ABSORB_GRID_MAX_BANDS == PCL_SCATTER_GRID_MAX_BANDS,
              "the absorber's grid and bands are the scattering medium's");

template <typename T>
struct gabsorb_args {
    const T *r[3];               // rows some axis needs (NULL otherwise)
    T *v[3], *dv[3];
    const T *E;                  // NULL without energy bands
    const unsigned char *kind;   // NULL: every particle is a photon
    const int64_t *ids;          // NULL: the id of slot i is id_base + i
    const double *tables;        // p [n_cells] (if has_p) | omega0 [n_cells] (if has_om) | the axes' edges (a radius axis: squared) | E edges; device
    unsigned long long *out;     // exposed, interacted, absorbed along the path, at the interaction | absorbed by cell [n_cells]; device, zeroed
    int64_t N, ts, id_base;      // particles, tile stride of the slab (elements), id of slot 0
    int tile_log;                // log2 of the tile length
    int n_axes, n_E;             // axes of the grid, B (0: one column for every energy, B' = 1)
    int n_edges, n_cells;        // every edge of the axes and of E; cells of the grid x B'
    int coord[PCL_GRID_MAX_AXES], n_bins[PCL_GRID_MAX_AXES], edge_at[PCL_GRID_MAX_AXES], E_at;
    int rows;                    // bit k: row k of r is read
    int has_p, has_om;           // which tables the call gave: uniform over the launch
    double c[3];
    uint32_t k0, k1, pass;       // Philox key (seed_lo, seed_hi), the step's own pass counter
};

template <typename T, bool kLds>
__global__ void __launch_bounds__(kBlock) k_absorb_grid(gabsorb_args<T> a) {
    extern __shared__ double s_mem[];                                  // edges | p, omega0 (LDS form, those given) | four counts | by cell (LDS form)
    const int nE = a.n_E, n_tab = (a.has_p ? 1 : 0) + (a.has_om ? 1 : 0), n_lds_c = kLds ? a.n_cells : 0;
    const int om_at = a.has_p ? a.n_cells : 0;                          // where omega0 starts behind p, in device memory and in LDS alike
    double *s_edges = s_mem;
    double *s_tab = s_mem + a.n_edges;
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_tab + n_tab * n_lds_c);
    uint32_t *s_cell = s_cnt + 4;
    const int n_cnt = 4 + n_lds_c;
    for (int k = threadIdx.x; k < a.n_edges; k += kBlock) s_edges[k] = a.tables[n_tab * a.n_cells + k];
    for (int k = threadIdx.x; k < n_tab * n_lds_c; k += kBlock) s_tab[k] = a.tables[k];
    for (int k = threadIdx.x; k < n_cnt; k += kBlock) s_cnt[k] = 0;    // (the cells follow the four counts)
    __syncthreads();
    const double *tab = kLds ? s_tab : a.tables;                        // (global form: read-only loads, the tables stay in L2)
    const double *s_E = s_edges + a.E_at;
    const int lane = threadIdx.x & 63;
    const int64_t stride = grid_stride(), n_round = whole_waves(a.N);   // (the ballots below need whole waves inside the loop)
    // wave-uniform, as in the scattering on a grid: the cell and the count of consecutive trips whose absorbed lanes all sat in that
    // one cell, not added yet (fewer than 2^32: kMaxSlotsPerWorkgroup).  Every bulk run starts with all photons in ONE cell, and adds
    // to one address serialise where they are carried out; so a run is added once.
    int run_cell = 0;
    uint32_t run_n = 0;
    auto flush_run = [&]() {
        if (lane == 0 && run_n) {
            if (kLds) atomicAdd(&s_cell[run_cell], run_n);
            else atomicAdd(&a.out[4 + run_cell], (unsigned long long)run_n);
        }
        run_n = 0;
    };
    for (int64_t i = first_slot(); i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        bool photon = in;
        if (photon && a.kind) photon = a.kind[i] != 0;                  // plain Objects are never touched
        // moving: at_rest, written out as in the scattering on a grid and negated -- -0.0 == 0, a NaN moves, v0 != 0 loads no more of v
        const bool go = photon && !((double)a.v[0][ti] == 0.0 && (double)a.v[1][ti] == 0.0 && (double)a.v[2][ti] == 0.0);
        int cell = -1;                                                  // (cell of the grid) * B' + e; -1: not exposed
        if (go) {
            double x[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if ((a.rows >> k) & 1) x[k] = (double)a.r[k][ti];       // fp32 widens exactly
            bool ok = true;
            int at = 0;
            for (int ax = 0; ax < a.n_axes; ++ax) {                     // k_position_grid's lines
                const int co = a.coord[ax], nb = a.n_bins[ax];
                const double *e = s_edges + a.edge_at[ax];
                double q;
                if (co == PCL_GRID_RADIUS) {   // q, unfused, in this order (the library is built with -ffp-contract=off)
                    const double dx = x[0] - a.c[0], dy = x[1] - a.c[1], dz = x[2] - a.c[2];
                    q = (dx * dx + dy * dy) + dz * dz;
                } else {
                    q = co == 0 ? x[0] : (co == 1 ? x[1] : x[2]);
                }
                ok = ok && q >= e[0] && q <= e[nb];                     // NaN and anything outside the axis's range are in no cell
                at = at * nb + bin_of(e, nb, q);
            }
            if (ok && nE > 0) {
                const double e = (double)a.E[ti];
                ok = e >= s_E[0] && e <= s_E[nE];                       // NaN and under/overflow: in no band
                at = at * nE + bin_of(s_E, nE, e);
            }
            if (ok) cell = at;
        }
        const bool exposed = cell >= 0;
        bool inter = false, gone_path = false, gone_hit = false;
        if (exposed) {
            if (a.has_om)                                               // interacted in this pass: the scatter kernels' mark (NaN != 0 is true)
                inter = (double)a.dv[0][ti] != 0.0 || (double)a.dv[1][ti] != 0.0 || (double)a.dv[2][ti] != 0.0;
            const uint64_t id = id_of(a.ids, a.id_base, i);
            if (a.has_p) {
                const double p = tab[cell];
                if (p > 0.0)                                            // a transparent cell draws nothing; u < 1: p == 1 absorbs everybody
                    gone_path = first_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kGridAbsorbPath, a.k0, a.k1)) < p;
            }
            if (inter && !gone_path) {
                const double om = tab[om_at + cell];
                if (om < 1.0)                                           // a conservative cell draws nothing; the sense of the ground's albedo draw
                    gone_hit = !(first_u53(pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, kGridAbsorbHit, a.k0, a.k1)) < om);
            }
        }
        const bool gone = gone_path || gone_hit;
        const unsigned long long m_gone = __ballot(gone);
        const uint32_t n_exp = (uint32_t)__popcll(__ballot(exposed)), n_int = (uint32_t)__popcll(__ballot(inter));
        const uint32_t n_path = (uint32_t)__popcll(__ballot(gone_path)), n_hit = (uint32_t)__popcll(__ballot(gone_hit));
        if (lane == 0 && n_exp) atomicAdd(&s_cnt[0], n_exp);
        if (lane == 0 && n_int) atomicAdd(&s_cnt[1], n_int);
        if (lane == 0 && n_path) atomicAdd(&s_cnt[2], n_path);
        if (lane == 0 && n_hit) atomicAdd(&s_cnt[3], n_hit);
        bool counted = false;                                           // this lane's absorption is in the wave's run
        if (m_gone) {                                                   // (wave-uniform)
            const int c0 = __shfl(cell, __ffsll((long long)m_gone) - 1);
            if (__ballot(gone && cell == c0) == m_gone) {               // every absorbed lane of the wave in one cell: one add of their count,
                if (c0 != run_cell) {                                   // put off while the next trips absorb in the same cell
                    flush_run();
                    run_cell = c0;
                }
                run_n += n_path + n_hit;
                counted = true;
            }
        }
        if (!gone) continue;    // lanes that are left alone wait at the loop's head: no ballot below this line
        if (!counted) {
            if (kLds) atomicAdd(&s_cell[cell], 1u);
            else atomicAdd(&a.out[4 + cell], 1ull);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {                                   // park, written out: at rest where it is; "did not scatter"
            a.v[k][ti] = (T)0.0;
            a.dv[k][ti] = (T)0.0;
        }
    }
    flush_run();
    __syncthreads();
    // pcl_sweep::flush_cells, written out, for the reason given in k_absorb_scattered: a further caller changes the older kernels
    for (int k = threadIdx.x; k < n_cnt; k += kBlock)
        if (s_cnt[k]) atomicAdd(&a.out[k], (unsigned long long)s_cnt[k]);
}

struct gabsorb_spec { // a call's arguments, checked; what the kernel compares against
    gscatter_spec g;            // the geometry, the bands and the first table given, by check_gscatter
    bool has_p = false, has_om = false;
    bool draws = false;         // some cell has p > 0 or omega0 < 1: the ids are needed
    std::vector<double> tables; // p (if given) | omega0 (if given) | the axes' edges (a radius axis: squared) | E edges
    size_t n_tab() const { return (size_t)has_p + (size_t)has_om; }
    size_t cells() const { return (size_t)4 + (size_t)g.n_p; }          // the four counts | by cell
    size_t lds_small() const { return (size_t)g.n_edges * sizeof(double) + 4 * sizeof(uint32_t); }             // the global form's
    size_t lds_whole() const { return lds_small() + (size_t)g.n_p * (n_tab() * sizeof(double) + sizeof(uint32_t)); }   // the LDS form's
    bool lds_form() const { return g.n_p <= kGridAbsorbLdsCells && lds_whole() <= kGridAbsorbLdsBytes; }
    spans out(int64_t *counts, int64_t *by_cell) const { return {{counts, 4}, {by_cell, (size_t)g.n_p}}; }
};

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.  The geometry,
// the bands and the values of a table by check_gscatter itself, handed the first table given: what that call refuses, this one does.
bool check_gabsorb(int n_axes, const int *coords, const int *n_bins, const double *edges, const double *center, int n_E,
                   const double *E_edges, const double *p, const double *omega0, const int64_t *counts_out, const int64_t *cells_out,
                   gabsorb_spec &s) {
    if (!p && !omega0) return false;
    if (!check_gscatter(n_axes, coords, n_bins, edges, center, n_E, E_edges, p ? p : omega0, 0, 0.0, counts_out, cells_out, s.g)) return false;
    s.has_p = p != nullptr; s.has_om = omega0 != nullptr;
    const size_t n_p = (size_t)s.g.n_p;
    s.tables.assign(s.g.tables.begin(), s.g.tables.begin() + n_p);      // the first table given
    for (size_t k = 0; k < n_p; ++k) {
        if (!(omega0 == nullptr || (omega0[k] >= 0.0 && omega0[k] <= 1.0))) return false;   // (NaN as well)
        s.draws = s.draws || (p && p[k] > 0.0) || (omega0 && omega0[k] < 1.0);
    }
    if (p && omega0) s.tables.insert(s.tables.end(), omega0, omega0 + n_p);
    s.tables.insert(s.tables.end(), s.g.tables.begin() + n_p, s.g.tables.end());            // the edges
    return true;
}

template <typename T>
int launch_gabsorb(pcl_ctx *ctx, const store_view &v, const gabsorb_spec &s, uint64_t seed, uint32_t pass, const staged &st) {
    gabsorb_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *vel = nullptr, *dv = nullptr;
        if ((s.g.rows >> k) & 1) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &vel));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DV0 + k, &dv));     // (what makes a lazy dv real: an absorbed photon's is written)
        a.r[k] = static_cast<const T *>(r); a.v[k] = static_cast<T *>(vel); a.dv[k] = static_cast<T *>(dv);
        a.c[k] = s.g.c[k];
    }
    // E is asked for only with energy bands: the pointer costs a wavelength-dependent scatter step its term cache (pcl_shell.hip).
    void *E = nullptr;
    if (s.g.n_E > 0) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_E, &E));
    a.E = static_cast<const T *>(E); a.kind = st.kind; a.ids = st.ids; a.tables = st.tables; a.out = st.out;
    a.N = v.N; a.ts = v.ts; a.id_base = st.id_base; a.tile_log = v.tile_log;
    a.n_axes = s.g.n_axes; a.n_E = s.g.n_E; a.n_edges = s.g.n_edges; a.n_cells = (int)s.g.n_p; a.E_at = s.g.E_at; a.rows = s.g.rows;
    for (int k = 0; k < s.g.n_axes; ++k) { a.coord[k] = s.g.coord[k]; a.n_bins[k] = s.g.n_bins[k]; a.edge_at[k] = s.g.edge_at[k]; }
    a.has_p = s.has_p; a.has_om = s.has_om;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.pass = pass;
    const bool lds_form = s.lds_form();
    const size_t lds = lds_form ? s.lds_whole() : s.lds_small();
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(lds));
    if (lds_form) hipLaunchKernelGGL((k_absorb_grid<T, true>), dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    else hipLaunchKernelGGL((k_absorb_grid<T, false>), dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int absorb_grid(pcl_ctx *ctx, int n_axes, const int *coords_host, const int *n_bins_host, const double *edges_host,
                const double *center_host, int n_E_bins, const double *E_edges_host, const double *p_host, const double *omega0_host,
                uint64_t seed, uint32_t pass, int64_t *counts_out_host, int64_t *cells_out_host) {
    gabsorb_spec s;
    if (!ctx || !check_gabsorb(n_axes, coords_host, n_bins_host, edges_host, center_host, n_E_bins, E_edges_host, p_host, omega0_host,
                               counts_out_host, cells_out_host, s))
        return bad_argument(ctx);
    const spans out = s.out(counts_out_host, cells_out_host);
    store_view v;
    staged st(ctx);
    PCL_SWEEP_TRY(open_store(ctx, PCL_V0, &v));
    zero_spans(out);
    if (v.N <= 0) return PCL_OK;
    PCL_SWEEP_TRY(stage(st, v, s.cells(), s.tables.data(), s.tables.size(), s.draws));   // the ids only if somebody may draw
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_gabsorb, ctx, v, s, seed, pass, st));
    return fetch(st, out);
}

int group_absorb_grid(pcl_group *group, int n_axes, const int *coords_host, const int *n_bins_host, const double *edges_host,
                      const double *center_host, int n_E_bins, const double *E_edges_host, const double *p_host, const double *omega0_host,
                      uint64_t seed, uint32_t pass, int64_t *counts_out_host, int64_t *cells_out_host) {
    gabsorb_spec s;                                                     // the arguments first: a refused call looks at no group
    if (!check_gabsorb(n_axes, coords_host, n_bins_host, edges_host, center_host, n_E_bins, E_edges_host, p_host, omega0_host,
                       counts_out_host, cells_out_host, s))
        return bad_argument(nullptr);
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    if (ctx.empty()) return bad_argument(nullptr);
    return sum_shards(ctx, s.out(counts_out_host, cells_out_host), [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_absorb_grid(one, n_axes, coords_host, n_bins_host, edges_host, center_host, n_E_bins, E_edges_host, p_host,
                                    omega0_host, seed, pass, p, p + 4);
    });
}

} // namespace

extern "C" {

int pcl_step_surface_reflect(pcl_ctx *ctx, double radius, const double *center_host, double albedo, int mode, double c, uint64_t seed,
                             uint32_t pass, int64_t *counts_out_host) {
    return guarded([&] { return surface_reflect(ctx, radius, center_host, albedo, mode, c, seed, pass, counts_out_host); });
}

int pcl_group_step_surface_reflect(pcl_group *group, double radius, const double *center_host, double albedo, int mode, double c,
                                   uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    return guarded([&] { return group_surface_reflect(group, radius, center_host, albedo, mode, c, seed, pass, counts_out_host); });
}

int pcl_step_phase_redirect(pcl_ctx *ctx, int phase, double g, double c, uint64_t seed, uint32_t pass, int64_t *count_out_host) {
    return guarded([&] { return phase_redirect(ctx, phase, g, c, seed, pass, count_out_host); });
}

int pcl_group_step_phase_redirect(pcl_group *group, int phase, double g, double c, uint64_t seed, uint32_t pass,
                                  int64_t *count_out_host) {
    return guarded([&] { return group_phase_redirect(group, phase, g, c, seed, pass, count_out_host); });
}

int pcl_step_absorb_scattered(pcl_ctx *ctx, int n_layers, const double *omega0_host, const double *edges_host, const double *center_host,
                              int n_E_bins, const double *E_edges_host, uint64_t seed, uint32_t pass, int64_t *counts_out_host,
                              int64_t *E_hist_out_host) {
    return guarded([&] {
        return absorb_scattered(ctx, n_layers, omega0_host, edges_host, center_host, n_E_bins, E_edges_host, seed, pass, counts_out_host,
                                E_hist_out_host);
    });
}

int pcl_group_step_absorb_scattered(pcl_group *group, int n_layers, const double *omega0_host, const double *edges_host,
                                    const double *center_host, int n_E_bins, const double *E_edges_host, uint64_t seed, uint32_t pass,
                                    int64_t *counts_out_host, int64_t *E_hist_out_host) {
    return guarded([&] {
        return group_absorb_scattered(group, n_layers, omega0_host, edges_host, center_host, n_E_bins, E_edges_host, seed, pass,
                                      counts_out_host, E_hist_out_host);
    });
}

int pcl_step_phase_layered(pcl_ctx *ctx, int n_laws, const int *kinds_host, const double *g_host, const int *n_bins_host,
                           const double *mu_host, const double *F_host, int n_layers, const double *cum_host, const double *edges_host,
                           const double *center_host, double c, uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    return guarded([&] {
        return phase_layered(ctx, n_laws, kinds_host, g_host, n_bins_host, mu_host, F_host, n_layers, cum_host, edges_host, center_host, c,
                             seed, pass, counts_out_host);
    });
}

int pcl_group_step_phase_layered(pcl_group *group, int n_laws, const int *kinds_host, const double *g_host, const int *n_bins_host,
                                 const double *mu_host, const double *F_host, int n_layers, const double *cum_host,
                                 const double *edges_host, const double *center_host, double c, uint64_t seed, uint32_t pass,
                                 int64_t *counts_out_host) {
    return guarded([&] {
        return group_phase_layered(group, n_laws, kinds_host, g_host, n_bins_host, mu_host, F_host, n_layers, cum_host, edges_host,
                                   center_host, c, seed, pass, counts_out_host);
    });
}

int pcl_step_recycle_spent(pcl_ctx *ctx, const pcl_source *src, double c, int at_rest, double top, const double *center_host, int n_E,
                           const double *cdf_host, const double *grid_host, uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    return guarded([&] {
        return recycle_spent(ctx, src, c, at_rest, top, center_host, n_E, cdf_host, grid_host, seed, pass, counts_out_host);
    });
}

int pcl_group_step_recycle_spent(pcl_group *group, const pcl_source *src, double c, int at_rest, double top, const double *center_host,
                                 int n_E, const double *cdf_host, const double *grid_host, uint64_t seed, uint32_t pass,
                                 int64_t *counts_out_host) {
    return guarded([&] {
        return group_recycle_spent(group, src, c, at_rest, top, center_host, n_E, cdf_host, grid_host, seed, pass, counts_out_host);
    });
}

int pcl_step_absorb_path(pcl_ctx *ctx, int n_layers, int n_E_bins, const double *p_host, const double *edges_host,
                         const double *center_host, const double *E_edges_host, uint64_t seed, uint32_t pass, int64_t *counts_out_host,
                         int64_t *cells_out_host) {
    return guarded([&] {
        return absorb_path(ctx, n_layers, n_E_bins, p_host, edges_host, center_host, E_edges_host, seed, pass, counts_out_host,
                           cells_out_host);
    });
}

int pcl_group_step_absorb_path(pcl_group *group, int n_layers, int n_E_bins, const double *p_host, const double *edges_host,
                               const double *center_host, const double *E_edges_host, uint64_t seed, uint32_t pass,
                               int64_t *counts_out_host, int64_t *cells_out_host) {
    return guarded([&] {
        return group_absorb_path(group, n_layers, n_E_bins, p_host, edges_host, center_host, E_edges_host, seed, pass, counts_out_host,
                                 cells_out_host);
    });
}

int pcl_step_reemit_parked(pcl_ctx *ctx, int n_layers, const double *edges_host, const double *center_host, const double *eta_host,
                           const int *lambertian_host, const int *table_offsets_host, const double *cdf_host, const double *grid_host,
                           double c, uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    return guarded([&] {
        return reemit_parked(ctx, n_layers, edges_host, center_host, eta_host, lambertian_host, table_offsets_host, cdf_host, grid_host, c,
                             seed, pass, counts_out_host);
    });
}

int pcl_group_step_reemit_parked(pcl_group *group, int n_layers, const double *edges_host, const double *center_host,
                                 const double *eta_host, const int *lambertian_host, const int *table_offsets_host,
                                 const double *cdf_host, const double *grid_host, double c, uint64_t seed, uint32_t pass,
                                 int64_t *counts_out_host) {
    return guarded([&] {
        return group_reemit_parked(group, n_layers, edges_host, center_host, eta_host, lambertian_host, table_offsets_host, cdf_host,
                                   grid_host, c, seed, pass, counts_out_host);
    });
}

int pcl_step_refract_surface(pcl_ctx *ctx, double radius, const double *center_host, double n_inside, double n_outside, int fresnel,
                             double c, uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    return guarded([&] { return refract_surface(ctx, radius, center_host, n_inside, n_outside, fresnel, c, seed, pass, counts_out_host); });
}

int pcl_group_step_refract_surface(pcl_group *group, double radius, const double *center_host, double n_inside, double n_outside,
                                   int fresnel, double c, uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    return guarded([&] {
        return group_refract_surface(group, radius, center_host, n_inside, n_outside, fresnel, c, seed, pass, counts_out_host);
    });
}

int pcl_step_ground_spectral(pcl_ctx *ctx, double radius, const double *center_host, int n_bands, const double *E_edges_host,
                             const double *albedo_host, const double *specular_host, double c, uint64_t seed, uint32_t pass,
                             int64_t *counts_out_host, int64_t *bands_out_host) {
    return guarded([&] {
        return ground_spectral(ctx, radius, center_host, n_bands, E_edges_host, albedo_host, specular_host, c, seed, pass, counts_out_host,
                               bands_out_host);
    });
}

int pcl_group_step_ground_spectral(pcl_group *group, double radius, const double *center_host, int n_bands, const double *E_edges_host,
                                   const double *albedo_host, const double *specular_host, double c, uint64_t seed, uint32_t pass,
                                   int64_t *counts_out_host, int64_t *bands_out_host) {
    return guarded([&] {
        return group_ground_spectral(group, radius, center_host, n_bands, E_edges_host, albedo_host, specular_host, c, seed, pass,
                                     counts_out_host, bands_out_host);
    });
}

int pcl_step_scatter_layered(pcl_ctx *ctx, int n_layers, int n_E_bins, const double *p_host, const double *edges_host,
                             const double *center_host, const double *E_edges_host, int first, double c, uint64_t seed, uint32_t pass,
                             int64_t *counts_out_host, int64_t *cells_out_host) {
    return guarded([&] {
        return scatter_layered(ctx, n_layers, n_E_bins, p_host, edges_host, center_host, E_edges_host, first, c, seed, pass, counts_out_host,
                               cells_out_host);
    });
}

int pcl_group_step_scatter_layered(pcl_group *group, int n_layers, int n_E_bins, const double *p_host, const double *edges_host,
                                   const double *center_host, const double *E_edges_host, int first, double c, uint64_t seed,
                                   uint32_t pass, int64_t *counts_out_host, int64_t *cells_out_host) {
    return guarded([&] {
        return group_scatter_layered(group, n_layers, n_E_bins, p_host, edges_host, center_host, E_edges_host, first, c, seed, pass,
                                     counts_out_host, cells_out_host);
    });
}

int pcl_step_scatter_grid(pcl_ctx *ctx, int n_axes, const int *coords_host, const int *n_bins_host, const double *edges_host,
                          const double *center_host, int n_E_bins, const double *E_edges_host, const double *p_host, int first, double c,
                          uint64_t seed, uint32_t pass, int64_t *counts_out_host, int64_t *cells_out_host) {
    return guarded([&] {
        return scatter_grid(ctx, n_axes, coords_host, n_bins_host, edges_host, center_host, n_E_bins, E_edges_host, p_host, first, c, seed,
                            pass, counts_out_host, cells_out_host);
    });
}

int pcl_group_step_scatter_grid(pcl_group *group, int n_axes, const int *coords_host, const int *n_bins_host, const double *edges_host,
                                const double *center_host, int n_E_bins, const double *E_edges_host, const double *p_host, int first,
                                double c, uint64_t seed, uint32_t pass, int64_t *counts_out_host, int64_t *cells_out_host) {
    return guarded([&] {
        return group_scatter_grid(group, n_axes, coords_host, n_bins_host, edges_host, center_host, n_E_bins, E_edges_host, p_host, first,
                                  c, seed, pass, counts_out_host, cells_out_host);
    });
}

int pcl_step_box_walls(pcl_ctx *ctx, const int *modes_host, const double *lo_host, const double *hi_host, int64_t *counts_out_host) {
    return guarded([&] { return box_walls(ctx, modes_host, lo_host, hi_host, counts_out_host); });
}

int pcl_group_step_box_walls(pcl_group *group, const int *modes_host, const double *lo_host, const double *hi_host,
                             int64_t *counts_out_host) {
    return guarded([&] { return group_box_walls(group, modes_host, lo_host, hi_host, counts_out_host); });
}

int pcl_step_phase_grid(pcl_ctx *ctx, int n_laws, const int *kinds_host, const double *g_host, const int *law_bins_host,
                        const double *mu_host, const double *F_host, int n_mixtures, const double *cum_host, int n_axes,
                        const int *coords_host, const int *n_bins_host, const double *edges_host, const double *center_host,
                        const unsigned char *mixture_host, int outside, double c, uint64_t seed, uint32_t pass,
                        int64_t *counts_out_host) {
    return guarded([&] {
        return phase_grid(ctx, n_laws, kinds_host, g_host, law_bins_host, mu_host, F_host, n_mixtures, cum_host, n_axes, coords_host,
                          n_bins_host, edges_host, center_host, mixture_host, outside, c, seed, pass, counts_out_host);
    });
}

int pcl_group_step_phase_grid(pcl_group *group, int n_laws, const int *kinds_host, const double *g_host, const int *law_bins_host,
                              const double *mu_host, const double *F_host, int n_mixtures, const double *cum_host, int n_axes,
                              const int *coords_host, const int *n_bins_host, const double *edges_host, const double *center_host,
                              const unsigned char *mixture_host, int outside, double c, uint64_t seed, uint32_t pass,
                              int64_t *counts_out_host) {
    return guarded([&] {
        return group_phase_grid(group, n_laws, kinds_host, g_host, law_bins_host, mu_host, F_host, n_mixtures, cum_host, n_axes,
                                coords_host, n_bins_host, edges_host, center_host, mixture_host, outside, c, seed, pass, counts_out_host);
    });
}

int pcl_step_absorb_grid(pcl_ctx *ctx, int n_axes, const int *coords_host, const int *n_bins_host, const double *edges_host,
                         const double *center_host, int n_E_bins, const double *E_edges_host, const double *p_host,
                         const double *omega0_host, uint64_t seed, uint32_t pass, int64_t *counts_out_host, int64_t *cells_out_host) {
    return guarded([&] {
        return absorb_grid(ctx, n_axes, coords_host, n_bins_host, edges_host, center_host, n_E_bins, E_edges_host, p_host, omega0_host, seed,
                           pass, counts_out_host, cells_out_host);
    });
}

int pcl_group_step_absorb_grid(pcl_group *group, int n_axes, const int *coords_host, const int *n_bins_host, const double *edges_host,
                               const double *center_host, int n_E_bins, const double *E_edges_host, const double *p_host,
                               const double *omega0_host, uint64_t seed, uint32_t pass, int64_t *counts_out_host,
                               int64_t *cells_out_host) {
    return guarded([&] {
        return group_absorb_grid(group, n_axes, coords_host, n_bins_host, edges_host, center_host, n_E_bins, E_edges_host, p_host,
                                 omega0_host, seed, pass, counts_out_host, cells_out_host);
    });
}

} // extern "C"
