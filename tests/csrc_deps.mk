# Included by every host harness Makefile (tests/hostemu, tests/*_host; by most through host_rules.mk): every header a harness could
# include. A library rebuilt too often is harmless; one rebuilt too rarely lets the tests pass against old code.
CSRC_DEPS = $(wildcard ../../artis_amd/csrc/*.h ../../artis_amd/csrc/*.inc ../../include/*.h)
