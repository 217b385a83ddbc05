# Shared by the tests/*_host harnesses that build one library per options preset: lib$(NAME)_<preset>.so from $(NAME).cc, one per options preset of $(PRESETS).
# Same FP flags as tests/hostemu.
include ../csrc_deps.mk
CXX ?= g++
CXXFLAGS = -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra -Wno-unused-parameter -Wno-unused-function -Wno-unused-variable -Wno-unknown-pragmas -pthread
upper = $(shell echo $(1) | tr a-z A-Z)
all: $(foreach p,$(PRESETS),lib$(NAME)_$(p).so)
lib$(NAME)_classic.so: $(DEPS)
	$(CXX) $(CXXFLAGS) -shared -o $@.tmp $(NAME).cc -lm && mv $@.tmp $@
lib$(NAME)_%.so: $(DEPS)
	$(CXX) $(CXXFLAGS) -DARTIS_PRESET_$(call upper,$*) -shared -o $@.tmp $(NAME).cc -lm && mv $@.tmp $@
clean:
	rm -f lib$(NAME)_*.so
