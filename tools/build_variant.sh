#!/bin/bash
# Build a variant of libcqlrec.so with extra -D flags (A/B-ing kernel parameters):
#   tools/build_variant.sh NAME -DQS_FUSED_VALU=48 ...   ->  replay_cql_amd/libcqlrec_NAME.so
# Run a tool against it with CQLREC_LIB=replay_cql_amd/libcqlrec_NAME.so.  Sources and per-file flags: replay_cql_amd/build.py.
cd "$(dirname "$0")/.." && exec python -m replay_cql_amd.build --variant "$@"
