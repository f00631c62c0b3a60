// xh_venv_sample.inc -- std::discrete_distribution's pick over a row held
// VStepShape's way, as statements: included inside the body of
// venv_act_kernel (venv_kernels.hip, "The pick") and of venv_heur_kernel
// (venv_heur_kernels.hip).  A fragment and not a function on purpose: as a
// __forceinline__ function the same statements compiled to other code in the
// act kernels (the restatement's loops unrolled differently; up to 12 more
// VGPRs at 128 bins, DESIGN.md 8), and the act kernels are to stay the code
// they were.
//
// Reads, from the including scope: S = VStepShape<B, D> and B; float
// p[S::BPL], the lane's probabilities; double lsum, their sum in bin order,
// and sd, the env's (seg_sum_d); uint32_t x, the env's stream (two draws are
// taken); lane, li, seg0, segmask.  Writes int choice.
  {
    const double u = canonical(x);  // discrete_distribution's two draws
    const double t = u * sd;
    double c = seg_scan_d<S::LPE>(lsum, lane) - lsum;  // the earlier lanes'
    int cnt = 0;
    bool near = false;
#pragma unroll
    for (int k = 0; k < S::BPL; ++k) {
      c += (double)p[k];
      // the env's last boundary is 1.0: never below u
      const bool last = li == S::LPE - 1 && k == S::BPL - 1;
      cnt += !last && c < t;
      near |= !last && fabs(c - t) < 1e-9 * sd;
    }
    choice = seg_sum_i<S::LPE>(cnt);
    if ((__ballot(near) & segmask) != 0) {  // the reference's order, exactly
      double s2 = 0.0;
      for (int l = 0; l < S::LPE; ++l)
#pragma unroll
        for (int k = 0; k < S::BPL; ++k)
          s2 += (double)wave_shfl(p[k], seg0 + l);
      double acc = 0.0;
      int c2 = B - 1;
      for (int l = 0; l < S::LPE; ++l)
#pragma unroll
        for (int k = 0; k < S::BPL; ++k) {
          const int j = l * S::BPL + k;
          const double qj = (double)wave_shfl(p[k], seg0 + l) / s2;
          acc = j == 0 ? qj : acc + qj;
          const double cpj = j == B - 1 ? 1.0 : acc;
          if (!(cpj < u) && j < c2) c2 = j;
        }
      choice = c2;
    }
  }
