// Cartesian -> spherical winds of one cell (reference utils/postprocessing.py:74-122,143-187), written once for
// post.hip (forecast post-processing) and climatology.hip (paradis_spherical_winds_inplace).
//
// fp64 from the fp32 values and the host-built double sin / cos of the cell's latitude and longitude, rounded once to
// fp32: what numpy gives the reference when the dataset's lat / lon are float64.  R * T stays float32, as numpy keeps a
// Python scalar times a float32 array.  Every including unit is compiled with -ffp-contract=off, so both give the same
// bits.
#pragma once

// (x, y, z) -> (u, v, w).  level: a pressure-level triple, w = dr/dt * pg / (R T) with pg = p * g in Pa m/s^2 and T the
// level's temperature; otherwise (the 10 m triple) w keeps the Cartesian z.
__device__ __forceinline__ void spherical_wind(float wx, float wy, float wz, float T, bool level, double pg, double sla,
                                               double cla, double slo, double clo, float& u, float& v, float& w) {
  const double X = (double)wx, Y = (double)wy, Z = (double)wz;
  u = (float)(-X * slo + Y * clo);
  v = (float)(-X * sla * clo - Y * sla * slo + Z * cla);
  if (level) {
    const float rt = 287.05f * T;         // numpy: R * temperature stays float32
    w = (float)((-X * cla * clo - Y * cla * slo - Z * sla) * (pg / (double)rt));
  } else {
    w = wz;                               // wind_z_10m keeps its Cartesian value
  }
}
