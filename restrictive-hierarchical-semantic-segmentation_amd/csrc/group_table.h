// The class tree's group table of one level as the entry points take it (compose.hip, distill.hip): consecutive groups of
// channels, each with its parent channel at the level above, validated on the host and copied into the launch.
#pragma once

#include "common.h"
#include "level_common.h"

struct Groups {
  int n;
  int parent[MAXC];
  int size[MAXC];
};

static int fill_groups(Groups& g, int ngroups, const int* parent, const int* size, int C, int Cprev, const char* who) {
  HRSEG_CHECK_ARG(ngroups >= 0 && ngroups <= MAXC && (ngroups == 0 || (parent && size)), "%s: bad group table", who);
  g.n = ngroups;
  int tot = 0;
  for (int i = 0; i < ngroups; ++i) {
    HRSEG_CHECK_ARG(parent[i] >= 0 && parent[i] < Cprev && size[i] > 0, "%s: group %d out of range", who, i);
    g.parent[i] = parent[i];
    g.size[i] = size[i];
    tot += size[i];
  }
  HRSEG_CHECK_ARG(tot == C || ngroups == 0, "%s: group sizes sum to %d, level has %d channels", who, tot, C);
  return 0;
}
