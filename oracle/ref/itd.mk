# oracle/ref/itd.mk -- builds oracle/_ref/<CFG>/ref_itd: the reference's own cleanup_itd, aggregate (ice_itd) and bound_state (ice_state)
# with the module closure and the recipe of oracle/ref/Makefile (its MODS, DEFS, FC, FFLAGS: -ffp-contract=off), compiled unmodified
# from the sources where they lie and linked with our driver oracle/ref/ref_itd.F90.  Nothing is copied into this repository; every
# output goes to oracle/_ref/, which is git-ignored.  Test infrastructure: it produces the fixtures tests/golden/ref_itd_*.npz
# (tests/golden/make_ref_itd.py).
#   make -f itd.mk CFG=name NX=.. NY=.. BX=.. BY=.. MXB=.. NCAT=..
include Makefile

itd: $(OUT)/ref_itd
.DEFAULT_GOAL := itd

$(OUT)/ref_itd: ref_itd.F90 itd.mk Makefile
	@test -d $(REF)/source || { echo "oracle/_ref: $(REF) is not present (it never is on the GPU box): nothing to build"; exit 1; }
	@mkdir -p $(OUT)/i
	@set -e; cd $(OUT)/i; trap 'cd ..; rm -rf i' EXIT; objs=""; \
	for m in $(MODS); do b=$$(basename $$m); \
	  cpp -P -traditional $(DEFS) $(REF)/$$m.F90 > $$b.f90; \
	  $(FC) $(FFLAGS) -w -c $$b.f90 -o $$b.o; objs="$$objs $$b.o"; done; \
	$(FC) $(FFLAGS) -w -I. -c $(CURDIR)/ref_itd.F90 -o ref_itd.o; \
	$(FC) -o ../ref_itd ref_itd.o $$objs
	@echo "built $(OUT)/ref_itd"
