// kernels_wls_tile.hip.h — the BODY of k_model_wls (kernels_wls.hip.h) and of the kernels of
// kernels_huber.hip.h: the tile loop they share, as text. It is included inside each kernel's braces and not
// called as a function: a call, even one always inlined, costs k_model_wls<float, float> 5 and
// k_model_wls<double, float> 4 registers (162 / 168 against the 157 / 164 of
// profiles/wls_kernel_resources.txt), and those four instantiations are to stay what they were.
//
// In scope where it is included: the types D and TS; the constants KIND (WL_WLS / WL_HUBER / WL_HIST) and
// HAS_H; a WlCtx cx; and, as the kernel's parameters or as locals, dst, Xp, Hp, Q, P, K, mp, woff, tav, tax,
// taw, tbv, tbx, tbw, flags and part. Without HAS_H, Hp / taw / tbw are not read. WL_HIST: dst / tav / tbv /
// part are not read and nothing is stored; cx.hist follows the typed image. part: one partial of the loss
// per workgroup, and for WL_HUBER a second, the clipped count, a grid further on. (No include guard.)
  extern __shared__ __attribute__((aligned(16))) unsigned char wl_lds[];
  const int RB = (K + 3) / 4;
  double *qs = reinterpret_cast<double *>(wl_lds);  // [4 RB][MW_LDQ]
  double(*img)[MV_TILE + 1] = reinterpret_cast<double(*)[MV_TILE + 1]>(qs + (size_t)4 * RB * MW_LDQ);
  int64_t *sav = reinterpret_cast<int64_t *>(img + MV_TILE), *sax = sav + MV_TILE, *saw = sax + MV_TILE,
          *sbv = saw + MV_TILE, *sbx = sbv + MV_TILE, *sbw = sbx + MV_TILE;
  TS(*simg)[MV_TILE + 1] = reinterpret_cast<TS(*)[MV_TILE + 1]>(sbw + MV_TILE);  // (one side along b only)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j16 = lane & 15;
  const int64_t A = mp.ga.count, B = mp.gb.count, a0 = (int64_t)blockIdx.x * MV_TILE;
  const int na = (int)min((int64_t)MV_TILE, A - a0);
  const bool a_unit = flags & WL_A_UNIT, vec_st = flags & WL_VEC_ST;
  const bool x_b = !(flags & WL_X_ALONG_A), h_b = HAS_H && !(flags & WL_H_ALONG_A),
             both_b = x_b && (h_b || !HAS_H);
  const int64_t nbt = (B + MV_TILE - 1) / MV_TILE;
  const WlSide<TS> X{Xp, sax, sbx, mp.roff, x_b, (flags & WL_X_UNIT) != 0, (flags & WL_X_VEC) != 0};
  const WlSide<TS> H{Hp, saw, sbw, woff, h_b, (flags & WL_H_UNIT) != 0, (flags & WL_H_VEC) != 0};

  for (int e = threadIdx.x; e < 4 * RB * MV_TILE; e += 256) {  // the Q image: 4 rows of k per pass
    const int k = e / MV_TILE, al = e % MV_TILE;
    qs[k * MW_LDQ + al] = (al < na && k < K) ? Q[a0 + al + mp.ldq * (int64_t)k] : 0.0;
  }
  if (threadIdx.x < MV_TILE) {
    const int i = threadIdx.x;
    if (KIND != WL_HIST) sav[i] = i < na ? tav[a0 + i] : 0;
    sax[i] = i < na ? tax[a0 + i] : 0;
    if (HAS_H) saw[i] = i < na ? taw[a0 + i] : 0;
  }
  if constexpr (KIND == WL_HIST) {
    cx.hist = reinterpret_cast<uint32_t *>(simg + ((x_b != h_b && HAS_H) ? MV_TILE : 0));
    for (int e = threadIdx.x; e < WL_HIST_BINS; e += 256) cx.hist[e] = 0;
  }
  // this lane's row b = 16 wave + j16 of tile tb_ in P (nullptr outside), and a chunk of it:
  // p[rb] = P[b, 4 (c0 + rb) + g] (0 outside)
  auto p_row = [&](int64_t tb_) -> const double * {
    const int64_t b_ = tb_ * MV_TILE + 16 * wave + j16;
    if (tb_ >= nbt || b_ >= B) return nullptr;
    const int64_t q_ = b_ / mp.pL;
    return P + ((b_ - q_ * mp.pL) + mp.pLK * q_);
  };
  auto p_chunk = [&](const double *row, int c0, double(&p)[MW_CH]) {
#pragma unroll
    for (int rb = 0; rb < MW_CH; rb++) {
      const int k_ = 4 * (c0 + rb) + g;
      p[rb] = (row && k_ < K) ? row[mp.pL * (int64_t)k_] : 0.0;
    }
  };
  int64_t nbv = 0, nbx = 0, nbw = 0;
  const int ib = (int)threadIdx.x - MV_TILE;  // threads 64..127: the b offsets, a tile ahead
  auto load_b = [&](int64_t tb_) {
    const int64_t bb = tb_ * MV_TILE + ib;
    const bool ok = ib >= 0 && ib < MV_TILE && tb_ < nbt && bb < B;
    if (KIND != WL_HIST) nbv = ok ? tbv[bb] : 0;
    nbx = ok ? tbx[bb] : 0;
    if (HAS_H) nbw = ok ? tbw[bb] : 0;
  };
  const double *prow = p_row(blockIdx.y);
  double pn[MW_CH];
  p_chunk(prow, 0, pn);
  load_b(blockIdx.y);
  __syncthreads();  // the Q image is complete

  for (int64_t tb = blockIdx.y; tb < nbt; tb += gridDim.y) {
    const int nb = (int)min((int64_t)MV_TILE, B - tb * MV_TILE);
    if (ib >= 0 && ib < MV_TILE) {
      sbv[ib] = nbv;
      sbx[ib] = nbx;
      sbw[ib] = nbw;
    }
    load_b(tb + gridDim.y);
    const double *pnext = p_row(tb + gridDim.y);
    mv_f64x4 d[4];
#pragma unroll
    for (int t = 0; t < 4; t++) d[t] = mv_f64x4{0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < RB; c0 += MW_CH) {
      double pa[MW_CH];
#pragma unroll
      for (int rb = 0; rb < MW_CH; rb++) pa[rb] = pn[rb];
      if (c0 + MW_CH < RB)
        p_chunk(prow, c0 + MW_CH, pn);
      else
        p_chunk(pnext, 0, pn);
#pragma unroll
      for (int rb = 0; rb < MW_CH; rb++) {
        if (c0 + rb < RB) {
          const double *qk = qs + (4 * (c0 + rb) + g) * MW_LDQ + j16;
#pragma unroll
          for (int t = 0; t < 4; t++)
            d[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[rb], qk[16 * t], d[t], 0, 0, 0);
        }
      }
    }
    prow = pnext;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) img[16 * wave + g + 4 * r][16 * t + j16] = d[t][r];
    __syncthreads();
    if (x_b || h_b) {  // the side views whose unit-stride run lies along b: lane index along b
      constexpr int NH = MV_TILE / 8;
      const int bl = lane;
      const int64_t x0 = X.off + sax[0] + sbx[0], h0 = HAS_H ? H.off + saw[0] + sbw[0] : 0;
#pragma unroll
      for (int hf = 0; hf < 2; hf++) {
        TS xv[NH], hv[NH];
#pragma unroll
        for (int i = 0; i < NH; i++) {
          const int al = wave + 4 * (NH * hf + i);
          const bool ok = al < na && bl < nb;
          if (x_b) xv[i] = Xp[ok ? X.off + sax[al] + sbx[bl] : x0];
          if (h_b) hv[i] = Hp[ok ? H.off + saw[al] + sbw[bl] : h0];
        }
#pragma unroll
        for (int i = 0; i < NH; i++) {
          const int al = wave + 4 * (NH * hf + i);
          if (both_b) {
            if (al < na && bl < nb)
              img[bl][al] = wl_apply<KIND>((double)xv[i], HAS_H ? (double)hv[i] : 1.0, img[bl][al], cx);
          } else {
            simg[bl][al] = x_b ? xv[i] : hv[i];
          }
        }
      }
      __syncthreads();
    }
    if (vec_st)
      wl_store<D, TS, 16 / sizeof(D), KIND, HAS_H>(dst, mp, img, simg, sav, sbv, X, H, a0, na, nb, a_unit, both_b,
                                                   cx);
    else
      wl_store<D, TS, 1, KIND, HAS_H>(dst, mp, img, simg, sav, sbv, X, H, a0, na, nb, a_unit, both_b, cx);
    __syncthreads();  // the images and the b offsets are rewritten by the next tile
  }
  if constexpr (KIND != WL_HIST) {  // (a histogram kernel flushes cx.hist itself)
    const double acc = block_sum(cx.acc, &img[0][0]);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
  }
  if constexpr (KIND == WL_HUBER) {
    const double n = block_sum(cx.nclip, &img[0][0]);
    if (threadIdx.x == 0) part[((int64_t)gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = n;
  }
