// What more than one of the level units (head.hip, compose.hip, loss.hip, targets.hip) needs.
#pragma once

#define MAXC 16   // channels of one level of the class tree, at most

// grid of a grid-stride kernel of 256-thread blocks that gives a thread one pixel at a time: one block per 256 of the n
// pixels, at most `cap` blocks
static inline int pixel_blocks(long n, long cap) {
  const long blocks = (n + 255) / 256;
  return (int)(blocks > cap ? cap : blocks);
}
