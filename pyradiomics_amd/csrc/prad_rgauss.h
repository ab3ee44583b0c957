// prad_rgauss.h -- the coefficients of ITK's recursive Gaussian (itkRecursiveGaussianImageFilter.hxx SetUp /
// ComputeNCoefficients / ComputeDCoefficients / ComputeRemainingCoefficients, symmetric orders 0 and 2), worked out on the host
// and handed to the kernels by value: the single route (prad_filters.hip) and the batched one (prad_batch_log.hip) share them,
// so that both routes run their lines on the same twenty numbers.  Host only: no kernel lives here.
#pragma once

#include <cmath>

namespace prad {

struct RGaussCoef {
  double N0, N1, N2, N3, D1, D2, D3, D4, M1, M2, M3, M4, BN1, BN2, BN3, BN4, BM1, BM2, BM3, BM4;
};

inline void rgauss_n(double sigmad, double A1, double B1, double A2, double B2, double N[4], double &SN, double &DN, double &EN) {
  const double W1 = 0.6681, L1 = -1.3932, W2 = 2.0787, L2 = -1.3732;
  const double s1 = sin(W1 / sigmad), s2 = sin(W2 / sigmad), c1 = cos(W1 / sigmad), c2 = cos(W2 / sigmad);
  const double e1 = exp(L1 / sigmad), e2 = exp(L2 / sigmad);
  N[0] = A1 + A2;
  N[1] = e2 * (B2 * s2 - (A2 + 2 * A1) * c2);
  N[1] += e1 * (B1 * s1 - (A1 + 2 * A2) * c1);
  N[2] = (A1 + A2) * c2 * c1;
  N[2] -= B1 * c2 * s1 + B2 * c1 * s2;
  N[2] *= 2 * e1 * e2;
  N[2] += A2 * e1 * e1 + A1 * e2 * e2;
  N[3] = e2 * e1 * e1 * (B2 * s2 - A2 * c2);
  N[3] += e1 * e2 * e2 * (B1 * s1 - A1 * c1);
  SN = N[0] + N[1] + N[2] + N[3];
  DN = N[1] + 2 * N[2] + 3 * N[3];
  EN = N[1] + 4 * N[2] + 9 * N[3];
}

inline RGaussCoef rgauss_coefficients(double sigma, double spacing, int order, bool normalize) {
  const double W1 = 0.6681, L1 = -1.3932, W2 = 2.0787, L2 = -1.3732;
  const double A1[3] = {1.3530, -0.6724, -1.3563}, B1[3] = {1.8151, -3.4327, 5.2318};
  const double A2[3] = {-0.3531, 0.6724, 0.3446}, B2[3] = {0.0902, 0.6100, -2.2355};
  const double sigmad = sigma / fabs(spacing);
  const double c1 = cos(W1 / sigmad), c2 = cos(W2 / sigmad), e1 = exp(L1 / sigmad), e2 = exp(L2 / sigmad);
  double D[4];
  D[3] = e1 * e1 * e2 * e2;
  D[2] = -2 * c1 * e1 * e2 * e2;
  D[2] += -2 * c2 * e2 * e1 * e1;
  D[1] = 4 * c2 * c1 * e1 * e2;
  D[1] += e1 * e1 + e2 * e2;
  D[0] = -2 * (e2 * c2 + e1 * c1);
  const double SD = 1.0 + D[0] + D[1] + D[2] + D[3];
  const double DD = D[0] + 2 * D[1] + 3 * D[2] + 4 * D[3];
  const double ED = D[0] + 4 * D[1] + 9 * D[2] + 16 * D[3];
  double N[4], SN, DN, EN;
  if (order == 0) {
    rgauss_n(sigmad, A1[0], B1[0], A2[0], B2[0], N, SN, DN, EN);
    const double alpha0 = 2 * SN / SD - N[0];
    for (int i = 0; i < 4; i++) N[i] /= alpha0;
  } else {
    const double scale = normalize ? sigma * sigma : 1.0;
    double N0s[4], N2s[4], SN0, DN0, EN0, SN2, DN2, EN2;
    rgauss_n(sigmad, A1[0], B1[0], A2[0], B2[0], N0s, SN0, DN0, EN0);
    rgauss_n(sigmad, A1[2], B1[2], A2[2], B2[2], N2s, SN2, DN2, EN2);
    const double beta = -(2 * SN2 - SD * N2s[0]) / (2 * SN0 - SD * N0s[0]);
    for (int i = 0; i < 4; i++) N[i] = N2s[i] + beta * N0s[i];
    SN = SN2 + beta * SN0; DN = DN2 + beta * DN0; EN = EN2 + beta * EN0;
    const double alpha2 = (EN * SD * SD - ED * SN * SD - 2 * DN * DD * SD + 2 * DD * DD * SN) / (SD * SD * SD);
    for (int i = 0; i < 4; i++) N[i] = N[i] * scale / alpha2;
  }
  RGaussCoef c;
  c.N0 = N[0]; c.N1 = N[1]; c.N2 = N[2]; c.N3 = N[3];
  c.D1 = D[0]; c.D2 = D[1]; c.D3 = D[2]; c.D4 = D[3];
  c.M1 = N[1] - D[0] * N[0]; c.M2 = N[2] - D[1] * N[0]; c.M3 = N[3] - D[2] * N[0]; c.M4 = -D[3] * N[0];
  const double SNn = c.N0 + c.N1 + c.N2 + c.N3, SM = c.M1 + c.M2 + c.M3 + c.M4, SDd = 1.0 + D[0] + D[1] + D[2] + D[3];
  c.BN1 = D[0] * SNn / SDd; c.BN2 = D[1] * SNn / SDd; c.BN3 = D[2] * SNn / SDd; c.BN4 = D[3] * SNn / SDd;
  c.BM1 = D[0] * SM / SDd; c.BM2 = D[1] * SM / SDd; c.BM3 = D[2] * SM / SDd; c.BM4 = D[3] * SM / SDd;
  return c;
}

}  // namespace prad
