// orbfe_fast_emit.inc -- the survivors of one suppression row go to the wave's staging buffer, included TEXTUALLY by the dense body
// (orbfe_fast_body.inc) and the lane-compacting body (orbfe_fast_body_c.inc): the high or low pixel of either pair, then the low
// pixel of a pair that straddles a cell seam where both survived.  Expects in scope: g01 / g23 (!= 0 <=> survivor), m01 / m23,
// has01 / has23, b01 / b23 with their counts p01n / p23n, row_out, keyrow, ord_row, ordx[4], resp0, split01 / split23 / wave_split,
// sbuf, nbuf.  What differs between the two bodies stays with them: how keyrow and ordx are formed, and the flush of the staging
// buffer (the dense body flushes after the stores when the NEXT row might not fit, the compacting one before them when THIS row
// might not).
                if (has01) {
                    const bool hi = g01 > 0xFFFFu;
                    const uint32_t a = hi ? m01 >> 16 : m01 & 0xFFFFu;
                    sbuf[nbuf + lanes_below(b01)] = make_uint2(keyrow + (hi ? 1u : 0u) + ((a + resp0) << 24),
                                                               ord_row + (hi ? ordx[1] : ordx[0]));
                }
                if (has23) {
                    const bool hi = g23 > 0xFFFFu;
                    const uint32_t a = hi ? m23 >> 16 : m23 & 0xFFFFu;
                    sbuf[nbuf + p01n + lanes_below(b23)] = make_uint2(keyrow + (hi ? 3u : 2u) + ((a + resp0) << 24),
                                                                      ord_row + (hi ? ordx[3] : ordx[2]));
                }
                nbuf += p01n + p23n;
                if (wave_split) {  // both pixels of a seam pair survived: the low one is still to be written
                    const uint32_t gs = split01 ? g01 : (split23 ? g23 : 0u);
                    const bool dbl = row_out && (gs & 0xFFFFu) != 0u && gs > 0xFFFFu;
                    const unsigned long long bd = orb_ballot(dbl);
                    if (bd) {
                        if (dbl) {
                            const uint32_t a = (split23 ? m23 : m01) & 0xFFFFu;
                            sbuf[nbuf + lanes_below(bd)] = make_uint2(keyrow + (split23 ? 2u : 0u) + ((a + resp0) << 24),
                                                                      ord_row + (split23 ? ordx[2] : ordx[0]));
                        }
                        nbuf += __popcll(bd);
                    }
                }
