// k_soil_hydrology_body.h - the body of the soil hydrology kernels (k_soil_hydrology.hip includes it into k_soil_hydrology<FROST, ROF>
// and into k_soil_hydrology_lat, and nothing else may): sections A - H of include/elmk.h "soil hydrology", statement by statement as
// elmkernels_amd/hydrology.py: column() has them.  In scope where it is included: S, R, dt and the constants FROST, ROF and LAT.
// No include guard: it is included once per kernel.  FROST, ROF and LAT are compile-time constants that the including kernel supplies
// (template parameters, or constexpr locals): every `if constexpr` on them and the `LAT && lat` test of F.2 fold away in the forms
// that do not take them, and `lat` is [[maybe_unused]] for those forms.
  const gptr<double> rows = R.rows;
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ld = S->ld;
  if (c >= S->ncols) return;
#define SL(f, j) S->f[(int64_t)(NLEVSNO + (j)) * ld + c]  // soil layer j of a field that carries the snow levels
#define PL(f, j) S->f[(int64_t)(j) * ld + c]              // soil layer j of a soil-only field
#define ROW(r) rows[(int64_t)(r) * ld + c]

  double liq[HN], ice[HN], dz[HN], z[HN], zi[HN + 1], watsat[HN], sucsat[HN], bsw[HN], hksat[HN];
#pragma unroll
  for (int j = 0; j < HN; j++) {
    liq[j] = SL(h2osoi_liq, j);
    ice[j] = SL(h2osoi_ice, j);
    dz[j] = SL(dz, j);
    z[j] = SL(zsoi, j);
    watsat[j] = PL(watsat, j);
    sucsat[j] = PL(sucsat, j);
    bsw[j] = PL(bsw, j);
    hksat[j] = ROW(ELMK_HYD_HKSAT + j);
  }
#pragma unroll
  for (int j = 0; j <= HN; j++) zi[j] = SL(zisoi, j);  // zi[0] = the surface, zi[j + 1] = the bottom of layer j
  double zwt = ROW(ELMK_HYD_ZWT), wa = ROW(ELMK_HYD_WA), h2osfc = S->h2osfc[c];
  const double frac_h2osfc = S->frac_h2osfc[c], fsno = S->frac_sno_eff[c], top = S->qflx_top_soil[c];
  const int snl = S->snl[c];

  // A. ice and porosity
  double effpor[HN], icefrac[HN], vol_liq[HN], vol[HN], zmm[HN + 1], dzmm[HN + 1], zimm[HN + 1];
#pragma unroll
  for (int j = 0; j <= HN; j++) zimm[j] = zi[j] * 1.0e3;
#pragma unroll
  for (int j = 0; j < HN; j++) {
    const double vol_ice = dmin(watsat[j], ice[j] / (dz[j] * HY_DENICE));
    effpor[j] = dmax(0.01, watsat[j] - vol_ice);
    icefrac[j] = dmin(1.0, vol_ice / watsat[j]);
    vol_liq[j] = dmax(liq[j], 1.0e-6) / (dz[j] * HY_DENH2O);
    vol[j] = liq[j] / (dz[j] * HY_DENH2O) + ice[j] / (dz[j] * HY_DENICE);
    zmm[j] = z[j] * 1.0e3;
    dzmm[j] = dz[j] * 1.0e3;
  }
  zmm[HN] = 0.0;
  dzmm[HN] = 0.0;

  // B. surface runoff
  const double fsat = ROW(ELMK_HYD_WTFACT) * elmk_exp(-0.5 * HY_FFF_S * zwt);
  const double qflx_surf = fsat * top;

  // C. infiltration and h2osfc
  const double qevap = snl == 0 ? (double)S->qflx_evap_grnd[c] : (double)S->qflx_ev_soil[c];
  double q_in_soil = (1.0 - frac_h2osfc) * (top - qflx_surf);
  q_in_soil = q_in_soil - (1.0 - fsno - frac_h2osfc) * qevap;
  double q_in_sfc = frac_h2osfc * (top - qflx_surf);
  q_in_sfc = q_in_sfc - frac_h2osfc * S->qflx_ev_h2osfc[c];
  double m = elmk_pow(10.0, -HY_E_ICE * icefrac[0]) * hksat[0];
  m = dmin(m, elmk_pow(10.0, -HY_E_ICE * icefrac[1]) * hksat[1]);
  m = dmin(m, elmk_pow(10.0, -HY_E_ICE * icefrac[2]) * hksat[2]);
  const double qinmax = (1.0 - fsat) * m;
  const double excess = dmax(0.0, q_in_soil - (1.0 - frac_h2osfc) * qinmax);
  double infl = q_in_soil - excess;
  q_in_sfc = q_in_sfc + excess;
  const double frac_infclust = frac_h2osfc <= HY_PC ? 0.0 : elmk_pow(frac_h2osfc - HY_PC, HY_MU);
  const double thresh = ROW(ELMK_HYD_H2OSFC_THRESH);
  double qs = 0.0;
  if (h2osfc >= thresh) {
    qs = ROW(ELMK_HYD_K_WET) * frac_infclust * (h2osfc - thresh);
    qs = dmin(qs, (h2osfc - thresh) / dt);
  }
  if (qs < 1.0e-8) qs = 0.0;
  h2osfc = h2osfc + (q_in_sfc - qs) * dt;
  double drain_sfc;
  if (h2osfc < 0.0) {
    infl = infl + h2osfc / dt;
    h2osfc = 0.0;
    drain_sfc = 0.0;
  } else {
    drain_sfc = dmin(frac_h2osfc * qinmax, h2osfc / dt);
  }
  h2osfc = h2osfc - drain_sfc * dt;
  infl = infl + drain_sfc;
  if constexpr (ROF) {  // F1 - F3
    int64_t cr = c;
    asm volatile("" : "+v"(cr));
    const int32_t g = R.rof.cellof[cr];
    double wf = 0.0, ff = 0.0, ar = 0.0;
    if (g >= 0) {
      wf = R.rof.wf[g];
      ff = R.rof.ff[g];
      ar = R.rof.area[g];
    }
    double hr = 0.0, d = 0.0, fr = 0.0;
    if (g >= 0 && wf > 0.0 && ff > 0.0 && ar > 0.0) {
      hr = (wf / ar) * 1000.0;
      const double a = ff * qinmax, b = hr / dt;
      d = a < b ? a : b;
      fr = ff;
    }
    infl = infl + d;
    R.rof.out[(int64_t)ELMK_FPI_H2OROF * ld + cr] = hy_canon(hr);
    R.rof.out[(int64_t)ELMK_FPI_FRAC * ld + cr] = hy_canon(fr);
    R.rof.out[(int64_t)ELMK_FPI_QFLX_DRAIN * ld + cr] = hy_canon(d);
  }

  // D. soil water
  int jwt = HN;
#pragma unroll
  for (int j = HN - 1; j >= 0; j--)
    if (zwt <= zi[j + 1]) jwt = j;
  const double zwtmm = zwt * 1.0e3;
  double zq[HN + 1];
#pragma unroll
  for (int j = 0; j < HN; j++) {
    const double b1 = 1.0 - 1.0 / bsw[j];
    double ve;
    if (zwtmm <= zimm[j]) {
      ve = watsat[j];
    } else if (zwtmm < zimm[j + 1]) {
      const double t0 = elmk_pow((sucsat[j] + zwtmm - zimm[j]) / sucsat[j], b1);
      const double v1 = -sucsat[j] * watsat[j] / b1 / (zwtmm - zimm[j]) * (1.0 - t0);
      ve = (v1 * (zwtmm - zimm[j]) + watsat[j] * (zimm[j + 1] - zwtmm)) / (zimm[j + 1] - zimm[j]);
    } else {
      const double ti = elmk_pow((sucsat[j] + zwtmm - zimm[j + 1]) / sucsat[j], b1);
      const double t0 = elmk_pow((sucsat[j] + zwtmm - zimm[j]) / sucsat[j], b1);
      ve = -sucsat[j] * watsat[j] / b1 / (zimm[j + 1] - zimm[j]) * (ti - t0);
    }
    ve = dmin(watsat[j], dmax(ve, 0.0));
    zq[j] = dmax(HY_SMPMIN, -sucsat[j] * elmk_pow(dmax(ve / watsat[j], 0.01), -bsw[j]));
  }
  constexpr int L = HN - 1;
  zq[HN] = 0.0;
  if (jwt == HN) {
    const double b1 = 1.0 - 1.0 / bsw[L];
    const double t0 = elmk_pow((sucsat[L] + zwtmm - zimm[HN]) / sucsat[L], b1);
    double ve = -sucsat[L] * watsat[L] / b1 / (zwtmm - zimm[HN]) * (1.0 - t0);
    ve = dmin(watsat[L], dmax(ve, 0.0));
    zq[HN] = dmax(HY_SMPMIN, -sucsat[L] * elmk_pow(dmax(ve / watsat[L], 0.01), -bsw[L]));
    zmm[HN] = 0.5 * (zwtmm + zmm[L]);
    dzmm[HN] = zwtmm - zimm[HN];
  }
  double hk[HN], dhkdw[HN], imped[HN], smp[HN], dsmpdw[HN];
#pragma unroll
  for (int j = 0; j < HN; j++) {
    const int jp = j + 1 < HN ? j + 1 : HN - 1;
    const double s1 = dmin(1.0, 0.5 * (vol[j] + vol[jp]) / (0.5 * (watsat[j] + watsat[jp])));
    const double s2 = hksat[j] * elmk_pow(s1, 2.0 * bsw[j] + 2.0);
    imped[j] = elmk_pow(10.0, -HY_E_ICE * (0.5 * (icefrac[j] + icefrac[jp])));
    hk[j] = imped[j] * s1 * s2;
    dhkdw[j] = imped[j] * (2.0 * bsw[j] + 3.0) * s2 * (1.0 / (watsat[j] + watsat[jp]));
    const double sn = dmin(1.0, dmax(vol_liq[j] / watsat[j], 0.01));
    smp[j] = dmax(HY_SMPMIN, -sucsat[j] * elmk_pow(sn, -bsw[j]));
    dsmpdw[j] = -bsw[j] * smp[j] / (sn * watsat[j]);
  }
  // the interfaces: q[i] between nodes i and i + 1; interface HN - 1 is towards the aquifer node
  double q[HN], dq1[HN], dq2[HN];
#pragma unroll
  for (int i = 0; i < HN - 1; i++) {
    const double den = zmm[i + 1] - zmm[i];
    const double num = (smp[i + 1] - smp[i]) - (zq[i + 1] - zq[i]);
    q[i] = -hk[i] * num / den;
    dq1[i] = -(-hk[i] * dsmpdw[i] + num * dhkdw[i]) / den;
    dq2[i] = -(hk[i] * dsmpdw[i + 1] + num * dhkdw[i]) / den;
  }
  q[L] = dq1[L] = dq2[L] = 0.0;
  if (jwt == HN) {
    const double sn1 = dmin(1.0, dmax(vol[L] / watsat[L], 0.01));
    const double smp1 = dmax(HY_SMPMIN, -sucsat[L] * elmk_pow(sn1, -bsw[L]));
    const double dsmpdw1 = -bsw[L] * smp1 / (sn1 * watsat[L]);
    const double den = zmm[HN] - zmm[L];
    const double num = (smp1 - smp[L]) - (zq[HN] - zq[L]);
    q[L] = -hk[L] * num / den;
    dq1[L] = -(-hk[L] * dsmpdw[L] + num * dhkdw[L]) / den;
    dq2[L] = -(hk[L] * dsmpdw1 + num * dhkdw[L]) / den;
  }
  // the rows and the Thomas algorithm: forward elimination from row 0, then back substitution
  double gam[HN + 1], u[HN + 1];
  {
    double bet = dzmm[0] / dt + dq1[0];
    u[0] = (infl - q[0] - (double)PL(qflx_rootsoi, 0)) / bet;
    gam[0] = 0.0;
#pragma unroll
    for (int j = 1; j < HN; j++) {
      const double r = q[j - 1] - q[j] - (double)PL(qflx_rootsoi, j);
      const double a = -dq1[j - 1];
      const double b = dzmm[j] / dt - dq2[j - 1] + dq1[j];
      gam[j] = dq2[j - 1] / bet;
      bet = b - a * gam[j];
      u[j] = (r - a * u[j - 1]) / bet;
    }
    double r = 0.0, a = 0.0, b = 1.0;
    if (jwt == HN) {
      r = q[L];
      a = -dq1[L];
      b = dzmm[HN] / dt - dq2[L];
    }
    gam[HN] = dq2[L] / bet;
    bet = b - a * gam[HN];
    u[HN] = (r - a * u[L]) / bet;
#pragma unroll
    for (int j = HN - 1; j >= 0; j--) u[j] = u[j] - gam[j + 1] * u[j + 1];
  }
#pragma unroll
  for (int j = 0; j < HN; j++) liq[j] = liq[j] + u[j] * dzmm[j];
  // recharge
  double qcharge;
  if (jwt == HN) {
    qcharge = u[HN] * dzmm[HN] / dt;
  } else {
    // layer k = jwt and the layer above it (or 0), selected under a predicate
    double volk = 0.0, watk = 1.0, impk = 0.0, hksk = 0.0, bswk = 0.0, smpu = 0.0, zqu = 0.0, zup = 0.0;
    const int up = jwt - 1 > 0 ? jwt - 1 : 0;
#pragma unroll
    for (int j = 0; j < HN; j++) {
      if (j == jwt) {
        volk = vol[j];
        watk = watsat[j];
        impk = imped[j];
        hksk = hksat[j];
        bswk = bsw[j];
      }
      if (j == up) {
        smpu = smp[j];
        zqu = zq[j];
      }
      if (j == jwt - 1) zup = z[j];
    }
    const double sn = dmax(volk / watk, 0.01);
    const double ka = impk * hksk * elmk_pow(dmin(1.0, sn), 2.0 * bswk + 3.0);
    const double wh = smpu - zqu;
    if (jwt == 0) qcharge = -ka * (0.0 - wh) / ((zwt + 1.0e-3) * 1000.0);
    else qcharge = -ka * (0.0 - wh) / ((zwt - zup) * 1000.0 * 2.0);
    qcharge = dmax(-10.0 / dt, qcharge);
    qcharge = dmin(10.0 / dt, qcharge);
  }

  // E. water table
  {
    const double rous = hy_sy(zwt, watsat[L], sucsat[L], bsw[L]);
    if (jwt == HN) {
      wa = wa + qcharge * dt;
      zwt = zwt - qcharge * dt / 1000.0 / rous;
    } else {
      double qt = qcharge * dt;
      if (qt > 0.0) {
        bool done = false;
#pragma unroll
        for (int j = HN - 1; j >= 0; j--) {
          if (j <= jwt && !done) {
            const double sy = hy_sy(zwt, watsat[j], sucsat[j], bsw[j]);
            const double ql = dmax(0.0, dmin(qt, sy * (zwt - zi[j]) * 1.0e3));
            zwt = zwt - ql / sy / 1000.0;
            qt = qt - ql;
            if (qt <= 0.0) done = true;
          }
        }
      } else {
        bool done = false;
#pragma unroll
        for (int j = 0; j < HN; j++) {
          if (j >= jwt && !done) {
            const double sy = hy_sy(zwt, watsat[j], sucsat[j], bsw[j]);
            const double ql = dmin(0.0, dmax(qt, -(sy * (zi[j + 1] - zwt) * 1.0e3)));
            qt = qt - ql;
            if (qt >= 0.0) {
              zwt = zwt - ql / sy / 1000.0;
              done = true;
            } else {
              zwt = zi[j + 1];
            }
          }
        }
        if (qt < 0.0) zwt = zwt - qt / 1000.0 / rous;
      }
    }
  }
  jwt = HN;
#pragma unroll
  for (int j = HN - 1; j >= 0; j--)
    if (zwt <= zi[j + 1]) jwt = j;

  // F. drainage
  double rsub_top = 0.0;
  [[maybe_unused]] double ft = 0.0, zwp = 0.0, qp = 0.0;
  [[maybe_unused]] bool above = false;  // F'.A: the water table lies above the frost table, and F.1's rsub_top and F.2 are skipped
  if constexpr (FROST) {
    // An index the compiler cannot match with the loads at the top: what F' reads through it is loaded here, not carried across D and E.
    int64_t cf = c;
    asm volatile("" : "+v"(cf));
#define SLF(f, j) S->f[(int64_t)(NLEVSNO + (j)) * ld + cf]
    // dz and the ice are last used in A and next here, and effpor and icefrac follow from them: loaded and evaluated again (the same
    // operands, the same bits), so that their registers are free while the solve is at its widest
#pragma unroll
    for (int j = 0; j < HN; j++) {
      dz[j] = SLF(dz, j);
      ice[j] = SLF(h2osoi_ice, j);
      const double vol_ice = dmin(watsat[j], ice[j] / (dz[j] * HY_DENICE));
      effpor[j] = dmax(0.01, watsat[j] - vol_ice);
      icefrac[j] = dmin(1.0, vol_ice / watsat[j]);
    }
    // F'.0 the frost table: the first frozen layer under a thawed one
    int kf;
    bool frozen;
    {
      double t[HN];
#pragma unroll
      for (int j = 0; j < HN; j++) t[j] = SLF(t_soisno, j);
      kf = t[0] > HY_TFRZ ? HN - 1 : 0;
      bool found = false;
#pragma unroll
      for (int k = 1; k < HN; k++) {
        if (!found && t[k - 1] > HY_TFRZ && t[k] <= HY_TFRZ) {
          kf = k;
          found = true;
        }
      }
      double tk = t[0];
#pragma unroll
      for (int j = 1; j < HN; j++)
        if (j == kf) tk = t[j];
      frozen = tk <= HY_TFRZ;
    }
    ft = SLF(zsoi, kf);
    zwp = ft;
    above = zwt < ft && frozen;
    int jq = jwt, j0 = jwt;  // the conductivity is summed over jq .. kf, the water is taken from j0 .. kf
    double zw = zwt;         // the table the walk moves: zwt in A, zwp in B
    bool drains = above;
    if (!above) {
      // F'.B the perched table: the first layer from kf upwards at or below sat_lev, under saturated ones
      int kp = 0;
      bool found = false;
      double s1 = 0.0, s2 = 0.0, sb = 0.0, sbb = 0.0;  // v / watsat of kp and kp + 1; of the layer visited last and the one before
#pragma unroll
      for (int k = HN - 1; k >= 0; k--) {
        if (k <= kf && !found) {
          const double s = (liq[k] / (dz[k] * HY_DENH2O) + ice[k] / (dz[k] * HY_DENICE)) / watsat[k];
          if (s <= HY_SAT_LEV) {
            kp = k;
            found = true;
            s1 = s;
            s2 = sb;
          }
          sbb = sb;
          sb = s;
        }
      }
      if (!found) {  // kp = 0: the walk ended at layer 0
        s1 = sb;
        s2 = sbb;
      }
      if (!frozen) kp = kf;
      drains = kf > kp;
      if (drains) {
        const double zp = SLF(zsoi, kp), zp1 = SLF(zsoi, kp + 1);
        const double m = (zp1 - zp) / (s2 - s1);
        const double b = zp1 - m * s2;
        zwp = dmax(0.0, m * HY_SAT_LEV + b);
        zw = zwp;
      }
      jq = kp;
      j0 = kp + 1;
    }
    if (drains) {
      const double qpm = R.frows[(int64_t)ELMK_HYDF_Q_PERCH_MAX * ld + c];
      double qk = 0.0, ws = 0.0;
#pragma unroll
      for (int j = 0; j < HN; j++) {
        if (j >= jq && j <= kf) {
          const int jp = j + 1 < HN ? j + 1 : HN - 1;
          const double imp = elmk_pow(10.0, -HY_E_ICE * (0.5 * (icefrac[j] + icefrac[jp])));  // D.4's imped[j]
          qk = qk + imp * rows[(int64_t)(ELMK_HYD_HKSAT + j) * ld + cf] * dzmm[j];
          ws = ws + dzmm[j];
        }
      }
      if (ws > 0.0) qk = qk / ws;
      qp = qpm * qk * (ft - zw);
      double rt = -qp * dt;
      bool done = false;
#pragma unroll
      for (int j = 0; j < HN; j++) {
        if (j >= j0 && j <= kf && !done) {
          double rl = dmax(rt, -(liq[j] - HY_WATMIN));
          rl = dmin(rl, 0.0);
          rt = rt - rl;
          liq[j] = liq[j] + rl;
          if (rt >= 0.0) {
            zw = zw - rl / effpor[j] / 1000.0;
            done = true;
          } else {
            zw = zi[j + 1];
          }
        }
      }
      qp = qp + rt / dt;
      if (above) zwt = zw;
      else zwp = zw;
    }
  }
  if (!(FROST && above)) {
    const double rous = hy_sy(zwt, watsat[L], sucsat[L], bsw[L]);
    double si = 0.0, sd = 0.0;
    const int j0 = jwt - 1 > 0 ? jwt - 1 : 0;
#pragma unroll
    for (int j = 0; j < HN; j++) {
      if (j >= j0) {
        si = si + icefrac[j] * dzmm[j];
        sd = sd + dzmm[j];
      }
    }
    const double imp = elmk_pow(10.0, -HY_E_ICE * (si / sd));
    rsub_top = imp * ROW(ELMK_HYD_RSUB_TOP_MAX) * elmk_exp(-HY_FFF_D * zwt);
    [[maybe_unused]] bool lat = false;
    if constexpr (LAT) {  // L3: the net lateral flux in the place of the baseflow
      int64_t cl = c;
      asm volatile("" : "+v"(cl));
      lat = R.down[cl] != -2;
      if (lat) rsub_top = R.qnet[cl];
    }
    double rt = -rsub_top * dt;
    if (jwt == HN) {
      wa = wa + rt;
      zwt = zwt - rt / 1000.0 / rous;
      liq[L] = liq[L] + dmax(0.0, wa - HY_AQUIFER_MAX);
      wa = dmin(wa, HY_AQUIFER_MAX);
    } else if (LAT && lat && rt > 0.0) {  // a net inflow: E's rising walk, the water into the layers it passes
      bool done = false;
#pragma unroll
      for (int j = HN - 1; j >= 0; j--) {
        if (j <= jwt && !done) {
          const double sy = hy_sy(zwt, watsat[j], sucsat[j], bsw[j]);
          const double ql = dmax(0.0, dmin(rt, sy * (zwt - zi[j]) * 1.0e3));
          liq[j] = liq[j] + ql;
          zwt = zwt - ql / sy / 1000.0;
          rt = rt - ql;
          if (rt <= 0.0) done = true;
        }
      }
      liq[0] = liq[0] + rt;  // what is left stands at the surface; wa is untouched
    } else {
      bool done = false;
#pragma unroll
      for (int j = 0; j < HN; j++) {
        if (j >= jwt && !done) {
          const double sy = hy_sy(zwt, watsat[j], sucsat[j], bsw[j]);
          const double ql = dmin(0.0, dmax(rt, -(sy * (zi[j + 1] - zwt) * 1.0e3)));
          liq[j] = liq[j] + ql;
          rt = rt - ql;
          if (rt >= 0.0) {
            zwt = zwt - ql / sy / 1000.0;
            done = true;
          } else {
            zwt = zi[j + 1];
          }
        }
      }
      zwt = zwt - rt / 1000.0 / rous;
      wa = wa + rt;
    }
  }
  zwt = zwt < 0.0 ? 0.0 : zwt;
  zwt = 80.0 < zwt ? 80.0 : zwt;
#pragma unroll
  for (int j = HN - 1; j >= 1; j--) {
    const double cap = effpor[j] * dzmm[j];
    const double xs = dmax(liq[j] - cap, 0.0);
    liq[j] = dmin(cap, liq[j]);
    liq[j - 1] = liq[j - 1] + xs;
  }
  {
    const double xs1 = dmax(dmax(liq[0], 0.0) - dmax(0.0, watsat[0] * dzmm[0] - ice[0]), 0.0);
    liq[0] = liq[0] - xs1;
    h2osfc = h2osfc + xs1;
  }
  const double rsub_sat = 0.0;
#pragma unroll
  for (int j = 0; j < HN - 1; j++) {
    if (liq[j] < HY_WATMIN) {
      const double xs = HY_WATMIN - liq[j];
      liq[j] = liq[j] + xs;
      liq[j + 1] = liq[j + 1] - xs;
    }
  }
  if (liq[L] < HY_WATMIN) {
    double xs = HY_WATMIN - liq[L];
#pragma unroll
    for (int i = HN - 2; i >= 0; i--) {
      if (xs > 0.0) {
        const double avail = dmax(liq[i] - HY_WATMIN - xs, 0.0);
        const double take = dmin(avail, xs);
        liq[L] = liq[L] + take;
        liq[i] = liq[i] - take;
        xs = dmax(xs - take, 0.0);
      }
    }
    liq[L] = liq[L] + xs;
    rsub_top = rsub_top - xs / dt;
  }
  const double qflx_drain = rsub_sat + rsub_top;

  // G. top-layer dew and sublimation
  if (snl == 0) {
    liq[0] = liq[0] + (1.0 - frac_h2osfc) * S->qflx_dew_grnd[c] * dt;
    ice[0] = ice[0] + (1.0 - frac_h2osfc) * S->qflx_dew_snow[c] * dt;
    const double sub = S->qflx_sub_snow[c];
    if (sub * dt > ice[0]) ice[0] = 0.0;
    else ice[0] = ice[0] - (1.0 - frac_h2osfc) * sub * dt;
  }

  // H. stores
#pragma unroll
  for (int j = 0; j < HN; j++) {
    SL(h2osoi_liq, j) = liq[j];
    PL(h2osoi_vol, j) = liq[j] / (dz[j] * HY_DENH2O) + ice[j] / (dz[j] * HY_DENICE);
  }
  if (snl == 0) SL(h2osoi_ice, 0) = ice[0];
  S->h2osfc[c] = h2osfc;
  ROW(ELMK_HYD_ZWT) = hy_canon(zwt);
  ROW(ELMK_HYD_WA) = hy_canon(wa);
  ROW(ELMK_HYD_QFLX_SURF) = hy_canon(qflx_surf);
  ROW(ELMK_HYD_QFLX_INFL) = hy_canon(infl);
  ROW(ELMK_HYD_QFLX_H2OSFC_SURF) = hy_canon(qs);
  ROW(ELMK_HYD_QFLX_DRAIN) = hy_canon(qflx_drain);
  ROW(ELMK_HYD_QFLX_RSUB_SAT) = hy_canon(rsub_sat);
  ROW(ELMK_HYD_QCHARGE) = hy_canon(qcharge);
  ROW(ELMK_HYD_FSAT) = hy_canon(fsat);
  if constexpr (FROST) {
    R.frows[(int64_t)ELMK_HYDF_FROST_TABLE * ld + c] = hy_canon(ft);
    R.frows[(int64_t)ELMK_HYDF_ZWT_PERCHED * ld + c] = hy_canon(zwp);
    R.frows[(int64_t)ELMK_HYDF_QFLX_DRAIN_PERCHED * ld + c] = hy_canon(qp);
  }
#undef SL
#undef SLF
#undef PL
#undef ROW
